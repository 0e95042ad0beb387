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
// fh_qfedavg_rows reads them once.  The main kernel has the register-slot layout of rowslots.h:
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

#include "rowslots.h"

namespace fh {

constexpr int QFA_MAXC = 64;
constexpr int QFA_DEN_WAVES = 16;

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
    using vec_t = typename SlotVec<V>::type;
    __shared__ double red[4][NP];
    const int32_t* ip = row_index ? row_index : slots_identity;
    const uint32_t lane_off = threadIdx.x * V;
    double sq[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) sq[k] = 0.0;
    for (int64_t blk = blockIdx.x; blk * 256 < units; blk += gridDim.x) {
        if (blk * 256 + threadIdx.x >= units) break;  // only in the last tile of columns
        const int64_t col0 = begin + blk * (256 * V);
        vec_t raw[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k)
            raw[k] = slots_load<V>(rows, row_stride, ip, C, k, col0, lane_off);
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
            res[v] = canon_nan(acc);
        }
        *reinterpret_cast<vec_t*>(acc_out + col0 + lane_off) =
            *reinterpret_cast<const vec_t*>(res);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int slot;
    const double s = slots_wave_fold<NP>(sq, lane, &slot);
    if (slots_owner<NP>(lane)) red[wid][slot] = s;
    __syncthreads();
    if ((int)threadIdx.x < C) {
        const int k = threadIdx.x;
        part[(int64_t)k * nparts + part0 + blockIdx.x] = slots_block_sum(red, k);
    }
}

// One workgroup of 16 waves.  Wave w finishes clients w, w + 16, ... (part_sum).  Thread 0 then
// forms den left to right in fp64.
__global__ void __launch_bounds__(64 * QFA_DEN_WAVES)
qfedavg_den_kernel(const double* __restrict__ part, int nparts, const float* __restrict__ a,
                   const double* __restrict__ b, int C, double* __restrict__ sqdist,
                   double* __restrict__ state) {
    __shared__ double sq[QFA_MAXC];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int k = wid; k < C; k += QFA_DEN_WAVES) {
        const double s = part_sum(part, k, nparts, lane);
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
    return canon_nan(g + s);
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

// 16-B columns up to 16 slots, 8-B at 32, one column at 64: the values and the fp64 accumulators
// stay in registers.
static constexpr int qfa_vec(int NP) { return NP <= 16 ? 4 : (NP == 32 ? 2 : 1); }

template <int NP, int V>
static int qfa_launch(const float* rows, int64_t row_stride, const int32_t* row_index,
                      const float* a, int C, int64_t begin, int64_t units, const float* global,
                      float* acc, double* part, int nparts, int part0, hipStream_t st) {
    const int grid = slots_grid(units, NP);
    FH_LAUNCH((qfedavg_main_kernel<NP, V>), dim3(grid), dim3(256), 0, st, rows, row_stride,
              row_index, a, C, begin, units, global, acc, part, nparts, part0);
    FH_LAUNCH_CHECK("qfedavg_main");
    return FH_OK;
}

static int qfa_apply_launch(const float* acc_rows, int64_t row_stride, const int32_t* row_index,
                            int64_t P, const float* global, const double* state, float* out,
                            bool vec_ok, hipStream_t st) {
    int64_t done = 0;
    if (vec_ok && P >= 4) {
        const int64_t P4 = P / 4;
        FH_LAUNCH(qfedavg_apply_vec4_kernel, dim3(stream_grid(P4)), dim3(256), 0, st, acc_rows, row_stride,
                  row_index, P4, global, state, out);
        FH_LAUNCH_CHECK("qfedavg_apply_vec4");
        done = P4 * 4;
    }
    if (done < P) {
        FH_LAUNCH(qfedavg_apply_scalar_kernel, dim3(stream_grid(P - done)), dim3(256), 0, st, acc_rows, row_stride,
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
    const int NP = slots_np(num_clients);
    return pad16_floats(P) +
           (size_t)num_clients * (size_t)slots_parts_max(NP, qfa_vec(NP), P) * sizeof(double);
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
    if (mode == FH_QFA_FINISH) {
        if (P == 0) return FH_OK;
        FH_REQUIRE(rows && global && out, "qfedavg: null pointer");
        const bool vec_ok = (row_stride % 4 == 0) && aligned16(rows, global, out);
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
        part = reinterpret_cast<double*>(static_cast<char*>(workspace) + pad16_floats(P));
        const int NP = slots_np(C);
        const bool vec_ok = (row_stride % 4 == 0) && aligned16(rows, global, acc);
        const SlotsPlan plan = slots_plan(NP, qfa_vec(NP), vec_ok, P);
        nparts = plan.nparts;
        const int rc = slots_dispatch<QFA_MAXC, qfa_vec>(
            NP, plan, P, [&](auto np, auto v, int64_t begin, int64_t units, int part0) {
                return qfa_launch<decltype(np)::value, decltype(v)::value>(
                    rows, row_stride, row_index, a, C, begin, units, global, acc, part, nparts,
                    part0, st);
            });
        if (rc != FH_OK) return rc;
    }
    FH_LAUNCH(qfedavg_den_kernel, dim3(1), dim3(64 * QFA_DEN_WAVES), 0, st,
              static_cast<const double*>(part), nparts, a, b, C, sqdist, state);
    FH_LAUNCH_CHECK("qfedavg_den");
    if (mode == FH_QFA_STEP && P > 0) {
        const bool vec_ok = aligned16(acc, global, out);
        return qfa_apply_launch(acc, 0, nullptr, P, global, state, out, vec_ok, st);
    }
    return FH_OK;
}
