// fedopt.hip — adaptive server optimizers (Reddi et al., "Adaptive Federated Optimization",
// ICLR 2021): FedAvgM, FedAdagrad, FedAdam, FedYogi.  The reference repository assigns the
// aggregate to the global model; here the server steps the global model along the
// pseudo-gradient  d = aggregate - global  with first and second moments it keeps across
// rounds.  The definition lives in include/fedhip.h and DESIGN.md §5.
//
// fh_server_opt_step is one launch per round on the P-float parameter vector.  In rows mode
// (weights given) the aggregate is the FedAvg weighted sum of the client rows, formed in
// registers with exactly fedavg_vec4_kernel's rounding sequence and never written out; in
// single-row mode (weights NULL) the one row is an aggregate that already exists (an
// all-reduce, a robust rule, a secure-aggregation decode).  HBM-bound: reads (C+3)*P floats
// and writes 3*P ((C+2)*P and 2*P for FedAvgM, which has no second moment).  Each thread owns
// 4 consecutive coordinates (16-B loads / stores), the state loads are issued ahead of the
// client loop and four client rows are in flight at a time.  No workspace, atomics or LDS.
// Every operation is one rounded fp32 operation (the TU is built with -ffp-contract=off, no
// fmaf here); sqrtf and / are the correctly rounded ones, denormals are kept.
#include <cmath>

#include "fh_common.h"

namespace fh {

struct SoptScalars {
    float lr, beta1, beta2, omb1, omb2, tau;
};

// One coordinate: aggregate a, global g, moments m / v in, g' m' v' out (v untouched for
// FH_SOPT_MOMENTUM).  RULE is a compile-time constant: no per-coordinate branch on it.
template <int RULE>
__device__ __forceinline__ void sopt_coord(float a, float& g, float& m, float& v,
                                           const SoptScalars& s) {
    const float d = a - g;
    if (RULE == FH_SOPT_MOMENTUM) {
        const float bm = s.beta1 * m;
        const float mn = bm + d;
        const float st = s.lr * mn;
        g = canon_nan(g + st);
        m = canon_nan(mn);
        return;
    }
    const float bm = s.beta1 * m;
    const float od = s.omb1 * d;
    const float mn = bm + od;
    const float d2 = d * d;
    float vn;
    if (RULE == FH_SOPT_ADAGRAD) {
        vn = v + d2;
    } else if (RULE == FH_SOPT_ADAM) {
        const float bv = s.beta2 * v;
        const float o2 = s.omb2 * d2;
        vn = bv + o2;
    } else {
        const float t = v - d2;
        const float sg = t > 0.f ? 1.0f : (t < 0.f ? -1.0f : 0.0f);  // NaN t: 0
        const float o2 = s.omb2 * d2;
        const float os = o2 * sg;
        vn = v - os;
    }
    const float rt = sqrtf(vn);
    const float dn = rt + s.tau;
    const float q = mn / dn;
    const float st = s.lr * q;
    g = canon_nan(g + st);
    m = canon_nan(mn);
    v = canon_nan(vn);
}

// ROWS: a = (((0 + w0*x0) + w1*x1) + ...) over C rows; else a = the one row (C == 1).
template <int RULE, bool ROWS>
__global__ void __launch_bounds__(256)
server_opt_vec4_kernel(const float* __restrict__ rows, int64_t row_stride,
                       const int32_t* __restrict__ row_index, const float* __restrict__ weights,
                       int C, int64_t P4, float* __restrict__ global, float* __restrict__ m,
                       float* __restrict__ v, SoptScalars s) {
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < P4;
         q += (int64_t)gridDim.x * blockDim.x) {
        float4 g4 = reinterpret_cast<const float4*>(global)[q];
        float4 m4 = reinterpret_cast<const float4*>(m)[q];
        float4 v4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (RULE != FH_SOPT_MOMENTUM) v4 = reinterpret_cast<const float4*>(v)[q];
        float4 acc;
        if (ROWS) {
            acc = make_float4(0.f, 0.f, 0.f, 0.f);
            int k = 0;
            for (; k + 4 <= C; k += 4) {
                float4 x[4];
                float w[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t r = row_index ? row_index[k + u] : (k + u);
                    x[u] = reinterpret_cast<const float4*>(rows + r * row_stride)[q];
                    w[u] = weights[k + u];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    acc.x = acc.x + w[u] * x[u].x;
                    acc.y = acc.y + w[u] * x[u].y;
                    acc.z = acc.z + w[u] * x[u].z;
                    acc.w = acc.w + w[u] * x[u].w;
                }
            }
            for (; k < C; ++k) {
                const int64_t r = row_index ? row_index[k] : k;
                const float4 x = reinterpret_cast<const float4*>(rows + r * row_stride)[q];
                const float w = weights[k];
                acc.x = acc.x + w * x.x;
                acc.y = acc.y + w * x.y;
                acc.z = acc.z + w * x.z;
                acc.w = acc.w + w * x.w;
            }
        } else {
            const int64_t r = row_index ? row_index[0] : 0;
            acc = reinterpret_cast<const float4*>(rows + r * row_stride)[q];
        }
        sopt_coord<RULE>(acc.x, g4.x, m4.x, v4.x, s);
        sopt_coord<RULE>(acc.y, g4.y, m4.y, v4.y, s);
        sopt_coord<RULE>(acc.z, g4.z, m4.z, v4.z, s);
        sopt_coord<RULE>(acc.w, g4.w, m4.w, v4.w, s);
        reinterpret_cast<float4*>(global)[q] = g4;
        reinterpret_cast<float4*>(m)[q] = m4;
        if (RULE != FH_SOPT_MOMENTUM) reinterpret_cast<float4*>(v)[q] = v4;
    }
}

// Same bits, one coordinate per thread over [begin, P): odd strides, misaligned pointers and
// the P % 4 tail.
template <int RULE, bool ROWS>
__global__ void __launch_bounds__(256)
server_opt_scalar_kernel(const float* __restrict__ rows, int64_t row_stride,
                         const int32_t* __restrict__ row_index,
                         const float* __restrict__ weights, int C, int64_t begin, int64_t P,
                         float* __restrict__ global, float* __restrict__ m,
                         float* __restrict__ v, SoptScalars s) {
    for (int64_t j = begin + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < P;
         j += (int64_t)gridDim.x * blockDim.x) {
        float g1 = global[j], m1 = m[j], v1 = 0.f;
        if (RULE != FH_SOPT_MOMENTUM) v1 = v[j];
        float acc;
        if (ROWS) {
            acc = 0.f;
            for (int k = 0; k < C; ++k) {
                const int64_t r = row_index ? row_index[k] : k;
                acc = acc + weights[k] * rows[r * row_stride + j];
            }
        } else {
            const int64_t r = row_index ? row_index[0] : 0;
            acc = rows[r * row_stride + j];
        }
        sopt_coord<RULE>(acc, g1, m1, v1, s);
        global[j] = g1;
        m[j] = m1;
        if (RULE != FH_SOPT_MOMENTUM) v[j] = v1;
    }
}

template <int RULE, bool ROWS>
static int sopt_launch(const float* rows, int64_t row_stride, const int32_t* row_index,
                       const float* weights, int C, int64_t P, float* global, float* m, float* v,
                       const SoptScalars& s, bool vec_ok, hipStream_t st) {
    int64_t done = 0;
    if (vec_ok && P >= 4) {
        const int64_t P4 = P / 4;
        FH_LAUNCH((server_opt_vec4_kernel<RULE, ROWS>), dim3(stream_grid(P4)), dim3(256), 0, st,
                  rows, row_stride, row_index, weights, C, P4, global, m, v, s);
        FH_LAUNCH_CHECK("server_opt_vec4");
        done = P4 * 4;
    }
    if (done < P) {
        FH_LAUNCH((server_opt_scalar_kernel<RULE, ROWS>), dim3(stream_grid(P - done)), dim3(256), 0,
                  st, rows, row_stride, row_index, weights, C, done, P, global, m, v, s);
        FH_LAUNCH_CHECK("server_opt_scalar");
    }
    return FH_OK;
}

}  // namespace fh

using namespace fh;

extern "C" int fh_server_opt_step(const float* rows, int64_t row_stride, const int32_t* row_index,
                                  const float* weights, int32_t num_clients, int64_t P,
                                  float* global, float* m, float* v, int32_t rule,
                                  float server_lr, float beta1, float beta2, float tau,
                                  void* stream) {
    FH_REQUIRE(rule >= FH_SOPT_MOMENTUM && rule <= FH_SOPT_YOGI,
               "server_opt: rule=%d outside [0, 3]", rule);
    FH_REQUIRE(num_clients >= 1, "server_opt: num_clients=%d, need at least 1", num_clients);
    FH_REQUIRE(weights || num_clients == 1,
               "server_opt: no weights means one aggregate row, got num_clients=%d", num_clients);
    FH_REQUIRE(P >= 0 && row_stride >= 0, "server_opt: bad sizes P=%lld row_stride=%lld",
               (long long)P, (long long)row_stride);
    FH_REQUIRE(std::isfinite(server_lr) && std::isfinite(beta1) && std::isfinite(beta2) &&
                   std::isfinite(tau),
               "server_opt: non-finite scalar (server_lr=%g beta1=%g beta2=%g tau=%g)",
               (double)server_lr, (double)beta1, (double)beta2, (double)tau);
    FH_REQUIRE(tau >= 0.f, "server_opt: tau=%g is negative", (double)tau);
    if (P == 0) return FH_OK;
    FH_REQUIRE(rows && global && m && (v || rule == FH_SOPT_MOMENTUM),
               "server_opt: null pointer");
    hipStream_t st = as_stream(stream);
    SoptScalars s;
    s.lr = server_lr;
    s.beta1 = beta1;
    s.beta2 = beta2;
    s.omb1 = 1.0f - beta1;
    s.omb2 = 1.0f - beta2;
    s.tau = tau;
    const bool vec_ok = (row_stride % 4 == 0) && aligned16(rows, global, m) &&
                        (rule == FH_SOPT_MOMENTUM || aligned16(v));
    const bool by_rows = weights != nullptr;
#define FH_SOPT_CASE(r)                                                                        \
    case r:                                                                                    \
        return by_rows ? sopt_launch<r, true>(rows, row_stride, row_index, weights,            \
                                              num_clients, P, global, m, v, s, vec_ok, st)     \
                       : sopt_launch<r, false>(rows, row_stride, row_index, weights,           \
                                               num_clients, P, global, m, v, s, vec_ok, st);
    switch (rule) {
        FH_SOPT_CASE(FH_SOPT_MOMENTUM)
        FH_SOPT_CASE(FH_SOPT_ADAGRAD)
        FH_SOPT_CASE(FH_SOPT_ADAM)
        default:
            FH_SOPT_CASE(FH_SOPT_YOGI)
    }
#undef FH_SOPT_CASE
    return FH_OK;
}
