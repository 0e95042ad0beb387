// qfedavg.hip — q-FedAvg, fairness-aware aggregation (Li, Sanjabi, Beirami, Smith, "Fair Resource
// Allocation in Federated Learning", ICLR 2020, Algorithm 2).  The reference repository has only
// the sample-weighted FedAvg; the definitions live in include/fedhip.h and DESIGN.md §5.
//
// With the global model g the clients started from, client k's trained row x_k, its weight pi_k
// and its loss F_k, the host forms a_k = pi_k * F_k^q and b_k = pi_k * q * L * F_k^(q-1)
// (fedhip/ops.py qfedavg_coefficients) and the server sets
//     den   = sum_k ( b_k * ||x_k - g||^2 + a_k )
//     g_new = g + (1/den) * sum_k a_k * (x_k - g).
// den needs every client's squared distance to g, so built from the existing kernels the rule is
// fh_dpfa_row_sqnorm, a host read-back and fh_fednova_rows: the [C][P] rows are read twice.
// fh_qfedavg_rows reads them once.  The main kernel has center_iter_kernel's layout (center.hip):
// a thread keeps the C values of its V columns in registers (NP slots, a power of two, every
// register-array index a compile-time constant), turns them into the fp32 differences
// d_kj = x_kj - g_j, adds (double)d_kj^2 to its C fp64 accumulators and stores
// acc_j = sum_k a_k * d_kj.  HBM-bound: (C+1)*P floats read, P written.  A wave folds its
// accumulators with the halving butterfly, the workgroup's four waves are added in wave order and
// the partial goes to the workspace.  A second, one-workgroup launch adds the workgroups' partials
// in a fixed order and forms den in fp64, left to right; it stays on the device.  In STEP a third
// pass over acc and g (2*P floats read, P written) applies 1/den.  No atomics, no allocation, no
// host synchronisation: the bits are a function of C, P and the alignments only.  Every fp32
// operation is one rounded operation (the TU is built with -ffp-contract=off, no fmaf here);
// denormals are kept.
#include <cmath>

#include "fh_common.h"

namespace fh {

__device__ __forceinline__ float qfa_canon(float x) {  // one NaN out, as fednova.hip
    return (x != x) ? __uint_as_float(0x7FC00000u) : x;
}

// row_index == NULL reads this instead: one code path, no branch around the index load
__device__ const int32_t qfa_identity[64] = {
    0,  1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21,
    22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43,
    44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63};

template <int V> struct QfaVec;
template <> struct QfaVec<4> { using type = float4; };
template <> struct QfaVec<2> { using type = float2; };
template <> struct QfaVec<1> { using type = float; };

constexpr int QFA_MAXC = 64;
constexpr int QFA_DEN_WAVES = 16;

// Sum a[k] over the 64 lanes for every k < NP: center.hip's ci_wave_fold.  Stage t pairs lane l
// with l ^ (32 >> t): the lane with that bit clear keeps the lower half of the live slots, the
// other the upper half, each adds what its partner held of the half it keeps.  After log2(NP)
// stages a lane holds one slot, summed over 2^stages lanes; the remaining lane bits are a plain
// butterfly.  Returns that slot's wave total; *slot is its k.  A fixed order of additions.
template <int H, int O, int NP>
__device__ __forceinline__ void qfa_fold_stage(double (&a)[NP], int lane, int& k) {
    if constexpr (H >= 1) {
        const bool upper = (lane & O) != 0;
#pragma unroll
        for (int i = 0; i < H; ++i) {
            const double send = upper ? a[i] : a[i + H];
            const double keep = upper ? a[i + H] : a[i];
            a[i] = keep + __shfl_xor(send, O, 64);
        }
        if (upper) k += H;
        qfa_fold_stage<H / 2, O / 2, NP>(a, lane, k);
    }
}

template <int NP>
__device__ __forceinline__ double qfa_wave_fold(double (&a)[NP], int lane, int* slot) {
    int k = 0;
    qfa_fold_stage<NP / 2, 32, NP>(a, lane, k);
    double s = a[0];
#pragma unroll
    for (int o = 32 / NP; o >= 1; o /= 2) s += __shfl_xor(s, o, 64);
    *slot = k;
    return s;
}

// One thread: V consecutive columns starting at begin + (tile*256 + tid)*V, tiles blockIdx.x,
// blockIdx.x + gridDim.x, ...  V > 1 needs 4*V-byte aligned rows / global / acc (the host
// checks); V == 1 is the scalar path (any stride, any alignment, the tail).  acc is the
// workspace (STEP) or the caller's out (PARTIAL), never global.
// part[k * nparts + part0 + blockIdx.x].
template <int NP, int V>
__global__ void __launch_bounds__(256)
qfedavg_main_kernel(const float* __restrict__ rows, int64_t row_stride,
                    const int32_t* __restrict__ row_index, const float* __restrict__ a, int C,
                    int64_t begin, int64_t units, const float* __restrict__ global,
                    float* __restrict__ acc_out, double* __restrict__ part, int nparts,
                    int part0) {
    using vec_t = typename QfaVec<V>::type;
    __shared__ double red[4][NP];
    const int32_t* ip = row_index ? row_index : qfa_identity;
    const uint32_t lane_off = threadIdx.x * V;
    double sq[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) sq[k] = 0.0;
    for (int64_t blk = blockIdx.x; blk * 256 < units; blk += gridDim.x) {
        if (blk * 256 + threadIdx.x >= units) break;  // only in the last tile of columns
        const int64_t col0 = begin + blk * (256 * V);
        // All NP loads are issued before the first use, in straight-line code.  Slots past C
        // re-read row C-1 (a cache hit, no branch) and are never used.
        vec_t raw[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int64_t r = ip[k < C ? k : C - 1];
            raw[k] = *reinterpret_cast<const vec_t*>(rows + r * row_stride + col0 + lane_off);
        }
        const vec_t gv = *reinterpret_cast<const vec_t*>(global + col0 + lane_off);
        // raw[k] becomes d_k = fl32(x_k - g), which both sums use
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            if (k < C) {
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const float d = reinterpret_cast<const float*>(&raw[k])[v] -
                                    reinterpret_cast<const float*>(&gv)[v];
                    reinterpret_cast<float*>(&raw[k])[v] = d;
                    // (double)d * (double)d is exact in fp64 (48 significant bits), so the
                    // fused form rounds exactly once, as multiply-then-add would
                    sq[k] = fma((double)d, (double)d, sq[k]);
                }
            }
        }
        float res[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                if (k < C) {
                    const float c = a[k];
                    if (c != 0.0f) {  // +-0: the row is skipped, whatever it holds (wave-uniform)
                        const float t = c * reinterpret_cast<const float*>(&raw[k])[v];
                        acc = acc + t;
                    }
                }
            }
            res[v] = qfa_canon(acc);
        }
        *reinterpret_cast<vec_t*>(acc_out + col0 + lane_off) =
            *reinterpret_cast<const vec_t*>(res);
    }
    int slot;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const double s = qfa_wave_fold<NP>(sq, lane, &slot);
    if ((lane & (63 >> (31 - __builtin_clz(NP)))) == 0) red[wid][slot] = s;
    __syncthreads();
    if ((int)threadIdx.x < C) {
        const int k = threadIdx.x;
        const double v = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];  // wave order
        part[(int64_t)k * nparts + part0 + blockIdx.x] = v;
    }
}

// One workgroup of 16 waves.  Wave w takes clients w, w + 16, ...: lane i adds partials i,
// i + 64, ... in order, then the butterfly (center_sqdist_finish_kernel's order).  Thread 0
// then forms den left to right in fp64.
__global__ void __launch_bounds__(64 * QFA_DEN_WAVES)
qfedavg_den_kernel(const double* __restrict__ part, int nparts, const float* __restrict__ a,
                   const double* __restrict__ b, int C, double* __restrict__ sqdist,
                   double* __restrict__ state) {
    __shared__ double sq[QFA_MAXC];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int k = wid; k < C; k += QFA_DEN_WAVES) {
        double s = 0.0;
        for (int p = lane; p < nparts; p += 64) s += part[(int64_t)k * nparts + p];
        s = wave_sum(s);
        if (lane == 0) {
            sq[k] = s;
            sqdist[k] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double den = 0.0;
        int live = 0;
        for (int k = 0; k < C; ++k) {
            const float ak = a[k];
            double h = 0.0;  // a client that is not live adds +0
            if (ak != 0.0f) {
                const double m = b[k] * sq[k];
                h = m + (double)ak;
                ++live;
            }
            den = k == 0 ? h : den + h;
        }
        state[0] = den;
        state[1] = (double)live;
    }
}

// out = g + fl32(1/den) * acc, den read from the device.  Nothing is multiplied when the
// inverse is zero: out = g, bit for bit.
__device__ __forceinline__ float qfa_inv(const double* state) {
    const double den = state[0];
    return (isfinite(den) && den > 0.0) ? (float)(1.0 / den) : 0.f;
}

__device__ __forceinline__ float qfa_apply(float acc, float g, float inv) {
    if (inv == 0.f) return g;
    const float s = inv * acc;
    return qfa_canon(g + s);
}

// acc_rows + idx[0] * row_stride is the [P] sum (FINISH: the caller's one row; STEP: the
// workspace, row_stride 0).  global and out may be the same buffer: every thread reads what it
// needs of a coordinate before it stores it, so neither is declared __restrict__.
__global__ void __launch_bounds__(256)
qfedavg_apply_vec4_kernel(const float* acc_rows, int64_t row_stride,
                          const int32_t* __restrict__ row_index, int64_t P4, const float* global,
                          const double* __restrict__ state, float* out) {
    const float inv = qfa_inv(state);
    const float* acc = acc_rows + (row_index ? (int64_t)row_index[0] : 0) * row_stride;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < P4;
         q += (int64_t)gridDim.x * blockDim.x) {
        const float4 g4 = reinterpret_cast<const float4*>(global)[q];
        const float4 a4 = reinterpret_cast<const float4*>(acc)[q];
        float4 o;
        o.x = qfa_apply(a4.x, g4.x, inv);
        o.y = qfa_apply(a4.y, g4.y, inv);
        o.z = qfa_apply(a4.z, g4.z, inv);
        o.w = qfa_apply(a4.w, g4.w, inv);
        reinterpret_cast<float4*>(out)[q] = o;
    }
}

__global__ void __launch_bounds__(256)
qfedavg_apply_scalar_kernel(const float* acc_rows, int64_t row_stride,
                            const int32_t* __restrict__ row_index, int64_t begin, int64_t P,
                            const float* global, const double* __restrict__ state, float* out) {
    const float inv = qfa_inv(state);
    const float* acc = acc_rows + (row_index ? (int64_t)row_index[0] : 0) * row_stride;
    for (int64_t j = begin + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < P;
         j += (int64_t)gridDim.x * blockDim.x)
        out[j] = qfa_apply(acc[j], global[j], inv);
}

// Workgroups of a main launch over `units` threads' worth of columns: at most `cap`, every one
// with the same number of tiles (but the last ones).  A function of units and NP alone
// (center.hip's ci_grid and widths: what keeps values and accumulators in registers).
static inline int qfa_np(int C) {
    int NP = 2;
    while (NP < C) NP *= 2;
    return NP;
}
static inline int qfa_vec(int NP) { return NP <= 16 ? 4 : (NP == 32 ? 2 : 1); }
static inline int qfa_grid(int64_t units, int NP) {
    if (units <= 0) return 0;
    const int64_t cap = NP >= 32 ? 512 : (NP == 16 ? 1024 : 2048);
    const int64_t tiles = ceil_div(units, 256);
    return (int)ceil_div(tiles, ceil_div(tiles, cap));
}
static inline int qfa_parts_vec(int NP, int64_t P) {
    const int V = qfa_vec(NP);
    if (V == 1) return qfa_grid(P, NP);
    const int64_t vecP = P / 4 * 4;
    return qfa_grid(vecP / V, NP) + qfa_grid(P - vecP, NP);
}
static inline size_t qfa_acc_bytes(int64_t P) { return ((size_t)P * sizeof(float) + 15) / 16 * 16; }

template <int NP, int V>
static int qfa_launch(const float* rows, int64_t row_stride, const int32_t* row_index,
                      const float* a, int C, int64_t begin, int64_t units, const float* global,
                      float* acc, double* part, int nparts, int part0, hipStream_t st) {
    const int grid = qfa_grid(units, NP);
    FH_LAUNCH((qfedavg_main_kernel<NP, V>), dim3(grid), dim3(256), 0, st, rows, row_stride,
              row_index, a, C, begin, units, global, acc, part, nparts, part0);
    FH_LAUNCH_CHECK("qfedavg_main");
    return FH_OK;
}

constexpr int64_t QFA_GRID_CAP = 8192;  // as fednova's: one pass covers 8192*256*4 coordinates

static int qfa_apply_launch(const float* acc_rows, int64_t row_stride, const int32_t* row_index,
                            int64_t P, const float* global, const double* state, float* out,
                            bool vec_ok, hipStream_t st) {
    int64_t done = 0;
    if (vec_ok && P >= 4) {
        const int64_t P4 = P / 4;
        const int grid = (int)std::min<int64_t>(ceil_div(P4, 256), QFA_GRID_CAP);
        FH_LAUNCH(qfedavg_apply_vec4_kernel, dim3(grid), dim3(256), 0, st, acc_rows, row_stride,
                  row_index, P4, global, state, out);
        FH_LAUNCH_CHECK("qfedavg_apply_vec4");
        done = P4 * 4;
    }
    if (done < P) {
        const int grid = (int)std::min<int64_t>(ceil_div(P - done, 256), QFA_GRID_CAP);
        FH_LAUNCH(qfedavg_apply_scalar_kernel, dim3(grid), dim3(256), 0, st, acc_rows, row_stride,
                  row_index, done, P, global, state, out);
        FH_LAUNCH_CHECK("qfedavg_apply_scalar");
    }
    return FH_OK;
}

}  // namespace fh

using namespace fh;

// [acc: P floats, padded to 16 bytes][partials: num_clients * parts doubles]
extern "C" size_t fh_qfedavg_workspace(int32_t num_clients, int64_t P) {
    if (num_clients < 1 || num_clients > QFA_MAXC || P <= 0) return 0;
    const int NP = qfa_np(num_clients);
    const int parts = std::max(qfa_parts_vec(NP, P), qfa_grid(P, NP));
    return qfa_acc_bytes(P) + (size_t)num_clients * (size_t)parts * sizeof(double);
}

extern "C" int fh_qfedavg_rows(const float* rows, int64_t row_stride, const int32_t* row_index,
                               const float* a, const double* b, int32_t num_clients, int64_t P,
                               const float* global, int32_t mode, float* out, void* workspace,
                               size_t ws_bytes, double* sqdist, double* state, void* stream) {
    const int C = num_clients;
    FH_REQUIRE(mode >= FH_QFA_STEP && mode <= FH_QFA_FINISH, "qfedavg: mode=%d outside [0, 2]",
               mode);
    if (mode == FH_QFA_FINISH)
        FH_REQUIRE(C == 1, "qfedavg: FINISH takes the one all-reduced row, got num_clients=%d", C);
    else
        FH_REQUIRE(C >= 1 && C <= QFA_MAXC, "qfedavg: num_clients=%d outside [1, 64]", C);
    FH_REQUIRE(P >= 0 && row_stride >= 0, "qfedavg: bad sizes P=%lld row_stride=%lld",
               (long long)P, (long long)row_stride);
    FH_REQUIRE(state, "qfedavg: null state");
    hipStream_t st = as_stream(stream);
    auto al16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
    if (mode == FH_QFA_FINISH) {
        if (P == 0) return FH_OK;
        FH_REQUIRE(rows && global && out, "qfedavg: null pointer");
        const bool vec_ok = (row_stride % 4 == 0) && al16(rows) && al16(global) && al16(out);
        return qfa_apply_launch(rows, row_stride, row_index, P, global, state, out, vec_ok, st);
    }
    // den is formed from a, b and the distances whatever P is
    FH_REQUIRE(a && b && sqdist, "qfedavg: null a, b or sqdist");
    int nparts = 0;
    float* acc = nullptr;
    double* part = nullptr;
    if (P > 0) {
        FH_REQUIRE(rows && global && out, "qfedavg: null pointer");
        FH_REQUIRE(mode == FH_QFA_STEP || out != global,
                   "qfedavg: PARTIAL's out cannot be the global vector");
        const size_t need = fh_qfedavg_workspace(C, P);
        FH_REQUIRE(workspace && ws_bytes >= need && reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
                   "qfedavg: workspace of %zu bytes, %zu needed (8-byte aligned)", ws_bytes, need);
        acc = mode == FH_QFA_STEP ? static_cast<float*>(workspace) : out;
        part = reinterpret_cast<double*>(static_cast<char*>(workspace) + qfa_acc_bytes(P));
        const int NP = qfa_np(C);
        const bool vec_ok = (row_stride % 4 == 0) && al16(rows) && al16(global) && al16(acc);
        // 16-B columns up to 16 slots, 8-B at 32, one column at 64: the values and the fp64
        // accumulators stay in registers.  The scalar instances take what the
        // vector path cannot: odd strides, misaligned pointers, the P % 4 tail.
        const int64_t vecP = (vec_ok && qfa_vec(NP) > 1) ? P / 4 * 4 : 0;
        nparts = vecP ? qfa_parts_vec(NP, P) : qfa_grid(P, NP);
        const int vparts = vecP ? qfa_grid(vecP / qfa_vec(NP), NP) : 0;
        int rc = FH_OK;
#define FH_QFA_CASE(np, v)                                                                       \
    case np:                                                                                     \
        if (vecP)                                                                                \
            rc = qfa_launch<np, v>(rows, row_stride, row_index, a, C, 0, vecP / v, global, acc,  \
                                   part, nparts, 0, st);                                         \
        if (rc == FH_OK && vecP < P)                                                             \
            rc = qfa_launch<np, 1>(rows, row_stride, row_index, a, C, vecP, P - vecP, global,    \
                                   acc, part, nparts, vparts, st);                               \
        break;
        switch (NP) {
            FH_QFA_CASE(2, 4)
            FH_QFA_CASE(4, 4)
            FH_QFA_CASE(8, 4)
            FH_QFA_CASE(16, 4)
            FH_QFA_CASE(32, 2)
            default:
                rc = qfa_launch<64, 1>(rows, row_stride, row_index, a, C, 0, P, global, acc, part,
                                       nparts, 0, st);
        }
#undef FH_QFA_CASE
        if (rc != FH_OK) return rc;
    }
    FH_LAUNCH(qfedavg_den_kernel, dim3(1), dim3(64 * QFA_DEN_WAVES), 0, st,
              static_cast<const double*>(part), nparts, a, b, C, sqdist, state);
    FH_LAUNCH_CHECK("qfedavg_den");
    if (mode == FH_QFA_STEP && P > 0) {
        const bool vec_ok = al16(acc) && al16(global) && al16(out);
        return qfa_apply_launch(acc, 0, nullptr, P, global, state, out, vec_ok, st);
    }
    return FH_OK;
}
