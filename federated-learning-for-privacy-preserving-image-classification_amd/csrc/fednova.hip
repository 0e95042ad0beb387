// fednova.hip — FedNova normalised averaging (Wang et al., "Tackling the Objective
// Inconsistency Problem in Heterogeneous Federated Optimization", NeurIPS 2020).  The reference
// repository averages the trained rows with sample-count weights only; with uneven local step
// counts a_k that average drifts toward the clients that ran the most steps.  FedNova divides
// every client's delta by its step count before averaging and rescales the result:
//     x_new = g + tau_eff * sum_k (p_k / a_k) * (x_k - g),      tau_eff = sum_k p_k * a_k.
// The host forms coef[k] = fl32(p_k / a_k) and tau_eff (fedhip/ops.py fednova_coefficients); the
// definition of the fp32 arithmetic lives in include/fedhip.h and DESIGN.md §5.
//
// fh_fednova_rows is one launch on the P-float parameter vector, in one of three modes: STEP
// (the whole rule), PARTIAL (a rank's share of the normalised sum, to all-reduce) and FINISH
// (apply an all-reduced sum).  HBM-bound: STEP and PARTIAL read (C+1)*P floats and write P,
// FINISH reads 2*P and writes P.  As in fedavg_vec4_kernel each thread owns 4 consecutive
// coordinates (16-B loads / stores), the global load is issued ahead of the client loop and
// four client rows are in flight at a time.  No workspace, atomics or LDS.  Every operation is
// one rounded fp32 operation (the TU is built with -ffp-contract=off, no fmaf here); denormals
// are kept.
//
// global, out and (in FINISH) rows may be the same buffer: every thread reads all it needs of a
// coordinate before it stores that coordinate and no thread touches another's, so none of the
// three is declared __restrict__.
#include <cmath>

#include "fh_common.h"

namespace fh {

// acc = acc + coef * (x - g): a rounded subtract, a rounded multiply, a rounded add.
__device__ __forceinline__ float nova_term(float acc, float c, float x, float g) {
    const float d = x - g;
    const float t = c * d;
    return acc + t;
}

template <int MODE>
__device__ __forceinline__ float nova_finish(float acc, float g, float tau) {
    if (MODE == FH_NOVA_PARTIAL) return canon_nan(acc);
    const float s = tau * acc;
    return canon_nan(g + s);
}

template <int MODE>
__global__ void __launch_bounds__(256)
fednova_vec4_kernel(const float* rows, int64_t row_stride, const int32_t* __restrict__ row_index,
                    const float* __restrict__ coef, int C, int64_t P4, const float* global,
                    float tau, float* out) {
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < P4;
         q += (int64_t)gridDim.x * blockDim.x) {
        const float4 g4 = reinterpret_cast<const float4*>(global)[q];
        float4 acc;
        if (MODE == FH_NOVA_FINISH) {
            const int64_t r = row_index ? row_index[0] : 0;
            acc = reinterpret_cast<const float4*>(rows + r * row_stride)[q];
        } else {
            acc = make_float4(0.f, 0.f, 0.f, 0.f);
            int k = 0;
            for (; k + 4 <= C; k += 4) {
                float4 x[4];
                float c[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t r = row_index ? row_index[k + u] : (k + u);
                    x[u] = reinterpret_cast<const float4*>(rows + r * row_stride)[q];
                    c[u] = coef[k + u];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    acc.x = nova_term(acc.x, c[u], x[u].x, g4.x);
                    acc.y = nova_term(acc.y, c[u], x[u].y, g4.y);
                    acc.z = nova_term(acc.z, c[u], x[u].z, g4.z);
                    acc.w = nova_term(acc.w, c[u], x[u].w, g4.w);
                }
            }
            for (; k < C; ++k) {
                const int64_t r = row_index ? row_index[k] : k;
                const float4 x = reinterpret_cast<const float4*>(rows + r * row_stride)[q];
                const float c = coef[k];
                acc.x = nova_term(acc.x, c, x.x, g4.x);
                acc.y = nova_term(acc.y, c, x.y, g4.y);
                acc.z = nova_term(acc.z, c, x.z, g4.z);
                acc.w = nova_term(acc.w, c, x.w, g4.w);
            }
        }
        float4 o;
        o.x = nova_finish<MODE>(acc.x, g4.x, tau);
        o.y = nova_finish<MODE>(acc.y, g4.y, tau);
        o.z = nova_finish<MODE>(acc.z, g4.z, tau);
        o.w = nova_finish<MODE>(acc.w, g4.w, tau);
        reinterpret_cast<float4*>(out)[q] = o;
    }
}

// Same bits, one coordinate per thread over [begin, P): odd strides, misaligned pointers and
// the P % 4 tail.
template <int MODE>
__global__ void __launch_bounds__(256)
fednova_scalar_kernel(const float* rows, int64_t row_stride,
                      const int32_t* __restrict__ row_index, const float* __restrict__ coef,
                      int C, int64_t begin, int64_t P, const float* global, float tau,
                      float* out) {
    for (int64_t j = begin + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < P;
         j += (int64_t)gridDim.x * blockDim.x) {
        const float g = global[j];
        float acc;
        if (MODE == FH_NOVA_FINISH) {
            const int64_t r = row_index ? row_index[0] : 0;
            acc = rows[r * row_stride + j];
        } else {
            acc = 0.f;
            for (int k = 0; k < C; ++k) {
                const int64_t r = row_index ? row_index[k] : k;
                acc = nova_term(acc, coef[k], rows[r * row_stride + j], g);
            }
        }
        out[j] = nova_finish<MODE>(acc, g, tau);
    }
}

template <int MODE>
static int nova_launch(const float* rows, int64_t row_stride, const int32_t* row_index,
                       const float* coef, int C, int64_t P, const float* global, float tau,
                       float* out, bool vec_ok, hipStream_t st) {
    int64_t done = 0;
    if (vec_ok && P >= 4) {
        const int64_t P4 = P / 4;
        FH_LAUNCH((fednova_vec4_kernel<MODE>), dim3(stream_grid(P4)), dim3(256), 0, st, rows,
                  row_stride, row_index, coef, C, P4, global, tau, out);
        FH_LAUNCH_CHECK("fednova_vec4");
        done = P4 * 4;
    }
    if (done < P) {
        FH_LAUNCH((fednova_scalar_kernel<MODE>), dim3(stream_grid(P - done)), dim3(256), 0, st,
                  rows, row_stride, row_index, coef, C, done, P, global, tau, out);
        FH_LAUNCH_CHECK("fednova_scalar");
    }
    return FH_OK;
}

}  // namespace fh

using namespace fh;

extern "C" int fh_fednova_rows(const float* rows, int64_t row_stride, const int32_t* row_index,
                               const float* coef, int32_t num_clients, int64_t P,
                               const float* global, float tau_eff, int32_t mode, float* out,
                               void* stream) {
    FH_REQUIRE(mode >= FH_NOVA_STEP && mode <= FH_NOVA_FINISH, "fednova: mode=%d outside [0, 2]",
               mode);
    FH_REQUIRE(num_clients >= 1, "fednova: num_clients=%d, need at least 1", num_clients);
    FH_REQUIRE(mode != FH_NOVA_FINISH || num_clients == 1,
               "fednova: FINISH takes the one all-reduced row, got num_clients=%d", num_clients);
    FH_REQUIRE(P >= 0 && row_stride >= 0, "fednova: bad sizes P=%lld row_stride=%lld",
               (long long)P, (long long)row_stride);
    FH_REQUIRE(mode == FH_NOVA_PARTIAL || std::isfinite(tau_eff),
               "fednova: non-finite tau_eff=%g", (double)tau_eff);
    if (P == 0) return FH_OK;
    FH_REQUIRE(rows && global && out && (coef || mode == FH_NOVA_FINISH),
               "fednova: null pointer");
    hipStream_t st = as_stream(stream);
    const bool vec_ok = (row_stride % 4 == 0) && aligned16(rows, global, out);
    switch (mode) {
        case FH_NOVA_STEP:
            return nova_launch<FH_NOVA_STEP>(rows, row_stride, row_index, coef, num_clients, P,
                                             global, tau_eff, out, vec_ok, st);
        case FH_NOVA_PARTIAL:
            return nova_launch<FH_NOVA_PARTIAL>(rows, row_stride, row_index, coef, num_clients,
                                                P, global, tau_eff, out, vec_ok, st);
        default:
            return nova_launch<FH_NOVA_FINISH>(rows, row_stride, row_index, coef, num_clients, P,
                                               global, tau_eff, out, vec_ok, st);
    }
}
