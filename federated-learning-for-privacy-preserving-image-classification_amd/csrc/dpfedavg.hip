// dpfedavg.hip — central, client-level differential privacy at the aggregation step: DP-FedAvg
// (McMahan et al., "Learning Differentially Private Recurrent Language Models", ICLR 2018) with
// adaptive quantile clipping (Andrew et al., "Differentially Private Learning with Adaptive
// Clipping", NeurIPS 2021).  The reference repository has no counterpart: its DP is the local,
// per-client mechanism of dp.hip.  The definition lives in include/fedhip.h and DESIGN.md §5.
//
// A round is four steps on the packed [clients][P] rows, all on the device, no host sync:
//   fh_dpfa_row_sqnorm   n_k^2 = sum_j (double)fl32(x_kj - g_j)^2          reads (C+1)*P floats
//   fh_dpfa_clip_coef    b_k, s_k = fl32(fl32(min(1, C_t/n_k)) * fl32(1/m)), sum b, sigma_avg
//   fh_dpfa_clip_sum     out = g + ((sum_k s_k*(x_k - g)) + sigma_avg*N(0,1))  reads (C+1)*P, writes P
//   fh_dpfa_clip_update  C_{t+1} = C_t * exp(-eta * (bbar - gamma))
// Both passes over the rows are HBM-bound.  The norm pass runs a (clients, chunks) grid with
// fp64 partials in a workspace and a second small launch that adds them in a fixed order: no
// floating-point atomics, the same bits on every run.  The sum pass gives each thread 4
// consecutive coordinates (16-B loads / stores), reads g once, writes out once and keeps eight
// client rows in flight.  Every fp32 operation of the sum is one rounded operation (the TU is
// built with -ffp-contract=off, no fmaf here); denormals are kept.
#include <cmath>

#include "fh_common.h"

namespace fh {

// ---- norms ---------------------------------------------------------------------------------
constexpr int DPFA_NORM_THREADS = 256;
constexpr int64_t DPFA_CHUNK_VEC = 2048;  // float4 per chunk: 8 per thread
constexpr int64_t DPFA_MAX_CHUNKS = 2048;

// The chunking is a function of P alone: with the row's alignment it fixes the summation order.
static void dpfa_chunks(int64_t P, int& nchunks, int64_t& span4) {
    const int64_t nq = ceil_div(P, 4) + 1;  // + 1: a row 4..12 B off has a head and a tail
    nchunks = (int)std::min<int64_t>(std::max<int64_t>(ceil_div(nq, DPFA_CHUNK_VEC), 1),
                                     DPFA_MAX_CHUNKS);
    span4 = ceil_div(nq, nchunks);
}

__device__ __forceinline__ double dpfa_sq(float x, float g, bool sub) {
    const float d = sub ? (x - g) : x;
    return (double)d * (double)d;
}

// Block (k, c): chunk c of selected row k.  When the row and g sit at the same offset from a
// 16-B boundary: scalar head up to the boundary, float4 body, scalar tail (head and tail by
// chunk 0); otherwise scalar throughout.  ws[k * nchunks + c] = the chunk's fp64 sum.
__global__ void __launch_bounds__(DPFA_NORM_THREADS)
dpfa_sqnorm_partial_kernel(const float* __restrict__ rows, int64_t row_stride,
                           const int32_t* __restrict__ row_index,
                           const float* __restrict__ global, int64_t P, int64_t span4,
                           int nchunks, double* __restrict__ ws) {
    __shared__ double red[DPFA_NORM_THREADS / 64];
    const int k = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const int64_t r = row_index ? row_index[k] : k;
    const float* l = rows + r * row_stride;
    const float* g = global;
    const bool sub = g != nullptr;
    const unsigned mis = (unsigned)(((uintptr_t)l >> 2) & 3);
    const bool vec = !g || (unsigned)(((uintptr_t)g >> 2) & 3) == mis;
    double s = 0.0;
    if (vec) {
        const int64_t h = min(P, (int64_t)((4 - mis) & 3));  // scalar head [0, h)
        const int64_t nb = (P - h) / 4;                       // float4 body [h, h + 4 nb)
        const float4* l4 = reinterpret_cast<const float4*>(l + h);
        const float4* g4 = reinterpret_cast<const float4*>(g + h);
        const int64_t qe = min(nb, (int64_t)(c + 1) * span4);
#pragma unroll 4
        for (int64_t q = (int64_t)c * span4 + tid; q < qe; q += DPFA_NORM_THREADS) {
            const float4 x = l4[q];
            float4 gv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (sub) gv = g4[q];
            s += (dpfa_sq(x.x, gv.x, sub) + dpfa_sq(x.y, gv.y, sub)) +
                 (dpfa_sq(x.z, gv.z, sub) + dpfa_sq(x.w, gv.w, sub));
        }
        if (c == 0) {
            if (tid < h) s += dpfa_sq(l[tid], sub ? g[tid] : 0.f, sub);
            const int64_t j = h + 4 * nb + tid;  // scalar tail [h + 4 nb, P): at most 3
            if (j < P) s += dpfa_sq(l[j], sub ? g[j] : 0.f, sub);
        }
    } else {
        const int64_t e = min(P, (int64_t)(c + 1) * span4 * 4);
        for (int64_t j = (int64_t)c * span4 * 4 + tid; j < e; j += DPFA_NORM_THREADS)
            s += dpfa_sq(l[j], g[j], true);
    }
    s = wave_sum(s);
    const int lane = tid & 63, wid = tid >> 6;
    if (lane == 0) red[wid] = s;
    __syncthreads();
    if (tid == 0) {
        double v = 0.0;
        for (int w = 0; w < DPFA_NORM_THREADS / 64; ++w) v += red[w];  // wave order
        ws[(int64_t)k * nchunks + c] = v;
    }
}

// One wave per row: lane i adds chunks i, i + 64, ... in order, then the butterfly.
__global__ void __launch_bounds__(64)
dpfa_sqnorm_finish_kernel(const double* __restrict__ ws, int nchunks, double* __restrict__ out) {
    const int k = blockIdx.x;
    double s = 0.0;
    for (int c = threadIdx.x; c < nchunks; c += 64) s += ws[(int64_t)k * nchunks + c];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[k] = s;
}

// ---- clip coefficients and the clip-norm update --------------------------------------------
// state: FH_DPFA_STATE_DOUBLES doubles, see include/fedhip.h.  One block.
__global__ void __launch_bounds__(256)
dpfa_coef_kernel(const double* __restrict__ sq, int C, double m_total, float w, double z_delta,
                 double* __restrict__ state, float* __restrict__ scale,
                 int32_t* __restrict__ bits, float* __restrict__ sigma) {
    __shared__ int count;
    if (threadIdx.x == 0) count = 0;
    __syncthreads();
    const double Ct = state[FH_DPFA_CLIP];
    int mine = 0;
    for (int k = threadIdx.x; k < C; k += blockDim.x) {
        const double n = sqrt(sq[k]);
        const int b = n <= Ct;  // NaN n: 0
        const float c = (n > Ct) ? (float)(Ct / n) : 1.0f;  // n == 0, NaN n: 1
        scale[k] = c * w;
        bits[k] = b;
        mine += b;
    }
    if (mine) atomicAdd(&count, mine);  // integers: any order, the same sum
    __syncthreads();
    if (threadIdx.x == 0) {
        const float sg = (float)(z_delta * Ct / m_total);
        if (sigma) sigma[0] = sg;
        state[FH_DPFA_SIGMA] = (double)sg;
        state[FH_DPFA_BITSUM] = (double)count;
    }
}

// No __restrict__: on one rank bit_sum is &state[FH_DPFA_BITSUM] (read before any store here).
__global__ void dpfa_update_kernel(double* state, const double* bit_sum, double m_total,
                                   double gamma, double eta, double sigma_b, uint64_t seed) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double Ct = state[FH_DPFA_CLIP];
    double num = bit_sum[0], next = Ct;
    if (eta != 0.0) {
        float xi[4];
        gauss4(seed, FH_DPFA_STREAM_BIT, 0ull, xi);
        num += sigma_b * (double)xi[0];
    }
    const double bbar = num / m_total;
    if (eta != 0.0) next = Ct * exp(-eta * (bbar - gamma));
    state[FH_DPFA_BBAR] = bbar;
    state[FH_DPFA_NEXT] = next;
    state[FH_DPFA_PREV] = Ct;
    state[FH_DPFA_CLIP] = next;
}

// ---- clipped sum + noise -------------------------------------------------------------------
template <bool SUB>
__device__ __forceinline__ float dpfa_term(float acc, float s, float x, float g) {
    const float d = SUB ? (x - g) : x;
    const float p = s * d;
    return acc + p;
}

template <bool SUB>
__device__ __forceinline__ void dpfa_term4(float4& acc, float s, const float4& x,
                                           const float4& g) {
    acc.x = dpfa_term<SUB>(acc.x, s, x.x, g.x);
    acc.y = dpfa_term<SUB>(acc.y, s, x.y, g.y);
    acc.z = dpfa_term<SUB>(acc.z, s, x.z, g.z);
    acc.w = dpfa_term<SUB>(acc.w, s, x.w, g.w);
}

__device__ __forceinline__ float dpfa_out(float acc, float g, float nu, bool noisy, bool add_g) {
    const float t = noisy ? (acc + nu) : acc;
    return canon_nan(add_g ? (g + t) : t);
}

// One coordinate, rows one after the other: the partial last vector and the scalar kernel.
template <bool SUB>
__device__ __forceinline__ float dpfa_coord(const float* rows, int64_t row_stride,
                                            const int32_t* __restrict__ row_index,
                                            const float* __restrict__ scale, int C, int64_t j,
                                            float g) {
    float acc = 0.f;
    for (int k = 0; k < C; ++k) {
        const int64_t r = row_index ? row_index[k] : k;
        acc = dpfa_term<SUB>(acc, scale[k], rows[r * row_stride + j], g);
    }
    return acc;
}

// Thread q owns coordinates 4q .. 4q+3 = the four lanes of Philox counter lo = q.  rows, global
// and out carry no __restrict__: out may be global, or the one row.
template <bool SUB>
__global__ void __launch_bounds__(256)
dpfa_sum_vec4_kernel(const float* rows, int64_t row_stride, const int32_t* __restrict__ row_index,
                     const float* __restrict__ scale, int C, int64_t P, const float* global,
                     float* out, const float* __restrict__ sigma, const float* noise_in,
                     uint64_t seed, uint64_t stream_hi, int add_g_flag) {
    constexpr int U = 8;  // rows in flight
    const bool add_g = add_g_flag != 0;
    const bool noisy = noise_in != nullptr || sigma != nullptr;
    const float sg = sigma ? sigma[0] : 0.f;
    const int64_t nq = (P + 3) / 4;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < nq;
         q += (int64_t)gridDim.x * blockDim.x) {
        float nu[4] = {0.f, 0.f, 0.f, 0.f};
        if (noisy && !noise_in) {
            gauss4(seed, stream_hi, (uint64_t)q, nu);
#pragma unroll
            for (int u = 0; u < 4; ++u) nu[u] = sg * nu[u];
        }
        if (q * 4 + 4 <= P) {
            float4 g4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (global) g4 = reinterpret_cast<const float4*>(global)[q];
            if (noise_in) {
                const float4 n4 = reinterpret_cast<const float4*>(noise_in)[q];
                nu[0] = n4.x; nu[1] = n4.y; nu[2] = n4.z; nu[3] = n4.w;
            }
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            int k = 0;
            for (; k + U <= C; k += U) {
                float4 x[U];
                float s[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t r = row_index ? row_index[k + u] : (k + u);
                    x[u] = reinterpret_cast<const float4*>(rows + r * row_stride)[q];
                    s[u] = scale[k + u];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) dpfa_term4<SUB>(acc, s[u], x[u], g4);
            }
            if (k + 4 <= C) {
                float4 x[4];
                float s[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t r = row_index ? row_index[k + u] : (k + u);
                    x[u] = reinterpret_cast<const float4*>(rows + r * row_stride)[q];
                    s[u] = scale[k + u];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) dpfa_term4<SUB>(acc, s[u], x[u], g4);
                k += 4;
            }
            for (; k < C; ++k) {
                const int64_t r = row_index ? row_index[k] : k;
                const float4 x = reinterpret_cast<const float4*>(rows + r * row_stride)[q];
                dpfa_term4<SUB>(acc, scale[k], x, g4);
            }
            float4 o;
            o.x = dpfa_out(acc.x, g4.x, nu[0], noisy, add_g);
            o.y = dpfa_out(acc.y, g4.y, nu[1], noisy, add_g);
            o.z = dpfa_out(acc.z, g4.z, nu[2], noisy, add_g);
            o.w = dpfa_out(acc.w, g4.w, nu[3], noisy, add_g);
            reinterpret_cast<float4*>(out)[q] = o;
        } else {  // the partial last vector: P % 4 coordinates
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int64_t j = q * 4 + u;
                if (j < P) {
                    const float g1 = global ? global[j] : 0.f;
                    const float n1 = noise_in ? noise_in[j] : nu[u];
                    const float acc = dpfa_coord<SUB>(rows, row_stride, row_index, scale, C, j, g1);
                    out[j] = dpfa_out(acc, g1, n1, noisy, add_g);
                }
            }
        }
    }
}

// Same bits, one coordinate per thread: odd strides and misaligned pointers.
template <bool SUB>
__global__ void __launch_bounds__(256)
dpfa_sum_scalar_kernel(const float* rows, int64_t row_stride,
                       const int32_t* __restrict__ row_index, const float* __restrict__ scale,
                       int C, int64_t P, const float* global, float* out,
                       const float* __restrict__ sigma, const float* noise_in, uint64_t seed,
                       uint64_t stream_hi, int add_g_flag) {
    const bool add_g = add_g_flag != 0;
    const bool noisy = noise_in != nullptr || sigma != nullptr;
    const float sg = sigma ? sigma[0] : 0.f;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < P;
         j += (int64_t)gridDim.x * blockDim.x) {
        float n1 = 0.f;
        if (noise_in) {
            n1 = noise_in[j];
        } else if (noisy) {
            float nu[4];
            gauss4(seed, stream_hi, (uint64_t)(j >> 2), nu);
            const int u = (int)(j & 3);
            const float gz = u == 0 ? nu[0] : (u == 1 ? nu[1] : (u == 2 ? nu[2] : nu[3]));
            n1 = sg * gz;
        }
        const float g1 = global ? global[j] : 0.f;
        const float acc = dpfa_coord<SUB>(rows, row_stride, row_index, scale, C, j, g1);
        out[j] = dpfa_out(acc, g1, n1, noisy, add_g);
    }
}

template <bool SUB>
static int dpfa_sum_launch(const float* rows, int64_t row_stride, const int32_t* row_index,
                           const float* scale, int C, int64_t P, const float* global, float* out,
                           const float* sigma, const float* noise_in, uint64_t seed,
                           uint64_t stream_hi, int add_g, bool vec_ok, hipStream_t st) {
    if (vec_ok) {
        FH_LAUNCH((dpfa_sum_vec4_kernel<SUB>), dim3(stream_grid(ceil_div(P, 4))), dim3(256), 0, st,
                  rows, row_stride, row_index, scale, C, P, global, out, sigma, noise_in, seed,
                  stream_hi, add_g);
        FH_LAUNCH_CHECK("dpfa_sum_vec4");
    } else {
        FH_LAUNCH((dpfa_sum_scalar_kernel<SUB>), dim3(stream_grid(P)), dim3(256), 0, st, rows,
                  row_stride, row_index, scale, C, P, global, out, sigma, noise_in, seed, stream_hi,
                  add_g);
        FH_LAUNCH_CHECK("dpfa_sum_scalar");
    }
    return FH_OK;
}

}  // namespace fh

using namespace fh;

extern "C" size_t fh_dpfa_row_sqnorm_workspace(int32_t num_clients, int64_t P) {
    if (num_clients < 1 || P <= 0) return 0;
    int nchunks;
    int64_t span4;
    dpfa_chunks(P, nchunks, span4);
    return (size_t)num_clients * (size_t)nchunks * sizeof(double);
}

extern "C" int fh_dpfa_row_sqnorm(const float* rows, int64_t row_stride, const int32_t* row_index,
                                  const float* global, int32_t num_clients, int64_t P,
                                  void* workspace, size_t workspace_bytes, double* sqnorm,
                                  void* stream) {
    FH_REQUIRE(num_clients >= 1, "dpfa_row_sqnorm: num_clients=%d, need at least 1", num_clients);
    FH_REQUIRE(P >= 0 && row_stride >= 0, "dpfa_row_sqnorm: bad sizes P=%lld row_stride=%lld",
               (long long)P, (long long)row_stride);
    FH_REQUIRE(sqnorm && (rows || P == 0), "dpfa_row_sqnorm: null pointer");
    hipStream_t st = as_stream(stream);
    int nchunks = 0;
    if (P > 0) {
        const size_t need = fh_dpfa_row_sqnorm_workspace(num_clients, P);
        FH_REQUIRE(workspace && workspace_bytes >= need,
                   "dpfa_row_sqnorm: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        int64_t span4;
        dpfa_chunks(P, nchunks, span4);
        FH_LAUNCH(dpfa_sqnorm_partial_kernel, dim3(num_clients, nchunks),
                  dim3(DPFA_NORM_THREADS), 0, st, rows, row_stride, row_index, global, P, span4,
                  nchunks, static_cast<double*>(workspace));
        FH_LAUNCH_CHECK("dpfa_sqnorm_partial");
    }
    FH_LAUNCH(dpfa_sqnorm_finish_kernel, dim3(num_clients), dim3(64), 0, st,
              static_cast<const double*>(workspace), nchunks, sqnorm);
    FH_LAUNCH_CHECK("dpfa_sqnorm_finish");
    return FH_OK;
}

extern "C" int fh_dpfa_clip_coef(const double* sqnorm, int32_t num_clients, int32_t total_clients,
                                 double z_delta, double* state, float* scale, int32_t* bits,
                                 float* sigma, void* stream) {
    FH_REQUIRE(num_clients >= 1, "dpfa_clip_coef: num_clients=%d, need at least 1", num_clients);
    FH_REQUIRE(total_clients >= num_clients,
               "dpfa_clip_coef: total_clients=%d below num_clients=%d", total_clients,
               num_clients);
    FH_REQUIRE(std::isfinite(z_delta) && z_delta >= 0.0,
               "dpfa_clip_coef: noise multiplier %g is negative or non-finite", z_delta);
    FH_REQUIRE(sqnorm && state && scale && bits, "dpfa_clip_coef: null pointer");
    const float w = 1.0f / (float)total_clients;
    FH_LAUNCH(dpfa_coef_kernel, dim3(1), dim3(256), 0, as_stream(stream), sqnorm,
              (int)num_clients, (double)total_clients, w, z_delta, state, scale, bits, sigma);
    FH_LAUNCH_CHECK("dpfa_clip_coef");
    return FH_OK;
}

extern "C" int fh_dpfa_clip_update(double* state, const double* bit_sum, int32_t total_clients,
                                   double target_quantile, double clip_lr, double bit_noise,
                                   uint64_t seed, void* stream) {
    FH_REQUIRE(total_clients >= 1, "dpfa_clip_update: total_clients=%d, need at least 1",
               total_clients);
    FH_REQUIRE(target_quantile >= 0.0 && target_quantile <= 1.0,
               "dpfa_clip_update: target_quantile=%g outside [0, 1]", target_quantile);
    FH_REQUIRE(std::isfinite(clip_lr) && clip_lr >= 0.0 && std::isfinite(bit_noise) &&
                   bit_noise >= 0.0,
               "dpfa_clip_update: clip_lr=%g / bit_noise=%g negative or non-finite", clip_lr,
               bit_noise);
    FH_REQUIRE(state && bit_sum, "dpfa_clip_update: null pointer");
    FH_LAUNCH(dpfa_update_kernel, dim3(1), dim3(64), 0, as_stream(stream), state, bit_sum,
              (double)total_clients, target_quantile, clip_lr, bit_noise, seed);
    FH_LAUNCH_CHECK("dpfa_clip_update");
    return FH_OK;
}

extern "C" int fh_dpfa_clip_sum(const float* rows, int64_t row_stride, const int32_t* row_index,
                                const float* scale, int32_t num_clients, int64_t P,
                                const float* global, float* out, const float* sigma,
                                const float* noise_in, uint64_t seed, uint64_t stream_hi,
                                int32_t flags, void* stream) {
    FH_REQUIRE(num_clients >= 1, "dpfa_clip_sum: num_clients=%d, need at least 1", num_clients);
    FH_REQUIRE(P >= 0 && row_stride >= 0, "dpfa_clip_sum: bad sizes P=%lld row_stride=%lld",
               (long long)P, (long long)row_stride);
    FH_REQUIRE((flags & ~(FH_DPFA_ROWS_ARE_DELTAS | FH_DPFA_NO_GLOBAL_ADD)) == 0,
               "dpfa_clip_sum: unknown flags 0x%x", (unsigned)flags);
    FH_REQUIRE(global || (flags & FH_DPFA_ROWS_ARE_DELTAS),
               "dpfa_clip_sum: no global vector means the rows are deltas (flags=0x%x)",
               (unsigned)flags);
    if (P == 0) return FH_OK;
    FH_REQUIRE(rows && scale && out, "dpfa_clip_sum: null pointer");
    const bool vec_ok = (row_stride % 4 == 0) && aligned16(rows, global, out, noise_in);
    const int add_g = (global && !(flags & FH_DPFA_NO_GLOBAL_ADD)) ? 1 : 0;
    hipStream_t st = as_stream(stream);
    if (flags & FH_DPFA_ROWS_ARE_DELTAS)
        return dpfa_sum_launch<false>(rows, row_stride, row_index, scale, num_clients, P, global,
                                      out, sigma, noise_in, seed, stream_hi, add_g, vec_ok, st);
    return dpfa_sum_launch<true>(rows, row_stride, row_index, scale, num_clients, P, global, out,
                                 sigma, noise_in, seed, stream_hi, add_g, vec_ok, st);
}
