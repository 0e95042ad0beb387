// rowslots.h — the scaffolding shared by the aggregation kernels that hold one column of every
// client row in registers: trimmed_mean_kernel (robust.hip), center_iter_kernel (center.hip),
// qfedavg_main_kernel (qfedavg.hip) and fltrust_stats_kernel (fltrust.hip).
//
// A thread owns V consecutive columns and keeps the C values of each in NP register slots (NP a
// power of two >= C, every register-array index a compile-time constant).  A workgroup of 256
// threads walks tiles of 256*V columns, tiles blockIdx.x, blockIdx.x + gridDim.x, ...  The
// kernels that also reduce over columns keep NP fp64 accumulators per thread, fold them across
// the wave with a halving butterfly, add the workgroup's four waves in wave order and write one
// partial per slot and workgroup; a second launch adds the partials in a fixed order.  The host
// half decides the slot count, the grid and the number of partials.  All of it is a function
// of C, P and the alignments only, and every rule takes it from here, so the rules cannot drift
// apart in partial counts or addition order.  The vector width per NP is the caller's (it
// depends on what else the kernel keeps in registers); nothing here knows which rule it serves.
#pragma once

#include "fh_common.h"

namespace fh {

// ---- device side ---------------------------------------------------------------------------
// row_index == NULL reads this instead: one code path, no branch around the index load
__device__ const int32_t slots_identity[64] = {
    0,  1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21,
    22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43,
    44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63};

template <int V> struct SlotVec;
template <> struct SlotVec<4> { using type = float4; };
template <> struct SlotVec<2> { using type = float2; };
template <> struct SlotVec<1> { using type = float; };

// The V columns at col0 + lane_off of slot k's row.  A kernel fills its raw[NP] with these in one
// unrolled loop before the first use, so all NP loads are issued in straight-line code and every
// row is in flight at once.  Slots past C re-read row C-1 (a cache hit, no branch); the caller
// never uses them.  The row pointers are wave-uniform (SGPR base) and the lane adds one 32-bit
// offset, so the NP addresses cost no VGPRs.
template <int V>
__device__ __forceinline__ typename SlotVec<V>::type slots_load(const float* rows,
                                                                int64_t row_stride,
                                                                const int32_t* ip, int C, int k,
                                                                int64_t col0, uint32_t lane_off) {
    const int64_t r = ip[k < C ? k : C - 1];
    return *reinterpret_cast<const typename SlotVec<V>::type*>(rows + r * row_stride + col0 +
                                                               lane_off);
}

// Sum a[k] over the 64 lanes for every k < NP.  Stage t pairs lane l with l ^ (32 >> t): the
// lane with that bit clear keeps the lower half of the live slots, the other the upper half,
// each adds what its partner held of the half it keeps.  After log2(NP) stages a lane holds one
// slot, k = sum_t ((lane & (32 >> t)) ? NP >> (t+1) : 0), summed over 2^stages lanes; the
// remaining lane bits are a plain butterfly.  Returns that slot's wave total (in every lane that
// shares the lane's top log2(NP) bits); *slot is its k.  A fixed order of additions, NP - 1
// exchanges and not 6*NP.
template <int H, int O, int NP>  // one stage: H slots kept, partner lane ^ O (compile-time indices)
__device__ __forceinline__ void slots_fold_stage(double (&a)[NP], int lane, int& k) {
    if constexpr (H >= 1) {
        const bool upper = (lane & O) != 0;
#pragma unroll
        for (int i = 0; i < H; ++i) {
            const double send = upper ? a[i] : a[i + H];
            const double keep = upper ? a[i + H] : a[i];
            a[i] = keep + __shfl_xor(send, O, 64);
        }
        if (upper) k += H;
        slots_fold_stage<H / 2, O / 2, NP>(a, lane, k);
    }
}

template <int NP>
__device__ __forceinline__ double slots_wave_fold(double (&a)[NP], int lane, int* slot) {
    int k = 0;
    slots_fold_stage<NP / 2, 32, NP>(a, lane, k);
    double s = a[0];
#pragma unroll
    for (int o = 32 / NP; o >= 1; o /= 2) s += __shfl_xor(s, o, 64);
    *slot = k;
    return s;
}

// After slots_wave_fold the 64 / NP lanes that share the top log2(NP) lane bits hold the same
// total; the one with the low bits clear stores it.
template <int NP>
__device__ __forceinline__ bool slots_owner(int lane) {
    return (lane & (63 >> (31 - __builtin_clz(NP)))) == 0;
}

// The block epilogue: the owner lanes store their totals to the wave's row of a __shared__
// red[4][...]; after the barrier, entry i of the four waves, added in wave order.
template <int N>
__device__ __forceinline__ double slots_block_sum(const double (&red)[4][N], int i) {
    return ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

// One wave finishes one slot: lane i adds partials i, i + 64, ... in order, then the butterfly.
// The result is in every lane.
__device__ __forceinline__ double part_sum(const double* part, int slot, int nparts, int lane) {
    const double* row = part + (int64_t)slot * nparts;
    double s = 0.0;
    for (int p = lane; p < nparts; p += 64) s += row[p];
    return wave_sum(s);
}

// ---- host side -----------------------------------------------------------------------------
inline int slots_np(int C) {
    int NP = 2;
    while (NP < C) NP *= 2;
    return NP;
}

// Workgroups of a launch over `units` threads' worth of columns: at most `cap`, every one with
// the same number of tiles (but the last ones).  A function of units and NP alone.
inline int slots_grid(int64_t units, int NP) {
    if (units <= 0) return 0;
    const int64_t cap = NP >= 32 ? 512 : (NP == 16 ? 1024 : 2048);
    const int64_t tiles = ceil_div(units, 256);
    return (int)ceil_div(tiles, ceil_div(tiles, cap));
}

// Partials per slot of the vector path: P/4*4 columns, V at a time, plus the scalar tail.
inline int slots_parts_vec(int NP, int V, int64_t P) {
    if (V == 1) return slots_grid(P, NP);
    const int64_t vecP = P / 4 * 4;
    return slots_grid(vecP / V, NP) + slots_grid(P - vecP, NP);
}

// What a workspace holds per slot: the larger of the vector path's partials and the all-scalar
// path's, so its size depends on C and P only, not on the alignments.
inline int slots_parts_max(int NP, int V, int64_t P) {
    return std::max(slots_parts_vec(NP, V, P), slots_grid(P, NP));
}

// How one call splits its P columns: [0, vecP) through the V-wide instance (0: none), writing
// partials [0, vparts); [vecP, P) through the scalar instance, which takes what the vector path
// cannot (odd strides, misaligned pointers, the P % 4 tail), writing partials [vparts, nparts).
struct SlotsPlan {
    int64_t vecP;
    int nparts, vparts;
};

inline SlotsPlan slots_plan(int NP, int V, bool vec_ok, int64_t P) {
    SlotsPlan p;
    p.vecP = (vec_ok && V > 1) ? P / 4 * 4 : 0;
    p.nparts = p.vecP ? slots_parts_vec(NP, V, P) : slots_grid(P, NP);
    p.vparts = p.vecP ? slots_grid(p.vecP / V, NP) : 0;
    return p;
}

// Runs launch(integral_constant NP, integral_constant V, begin, units, part0) -> FH_* for the
// runtime np: the vector launch if plan.vecP, then the scalar launch at part0 = plan.vparts.
// Instances exist for NP = 2, 4, ... MAXNP; VEC(NP) is the caller's vector width.
template <int MAXNP, int (*VEC)(int), int NP = 2, typename F>
inline int slots_dispatch(int np, const SlotsPlan& plan, int64_t P, F&& launch) {
    if constexpr (NP < MAXNP) {
        if (np != NP) return slots_dispatch<MAXNP, VEC, NP * 2>(np, plan, P, launch);
    }
    constexpr int V = VEC(NP);
    using slots_c = std::integral_constant<int, NP>;
    int rc = FH_OK;
    if (plan.vecP)
        rc = launch(slots_c{}, std::integral_constant<int, V>{}, (int64_t)0, plan.vecP / V, 0);
    if (rc == FH_OK && plan.vecP < P)
        rc = launch(slots_c{}, std::integral_constant<int, 1>{}, plan.vecP, P - plan.vecP,
                    plan.vparts);
    return rc;
}

}  // namespace fh
