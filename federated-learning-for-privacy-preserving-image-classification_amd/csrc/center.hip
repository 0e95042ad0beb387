// center.hip — the two robust rules that iterate a weighted sum of rows around a centre:
// the geometric median by the smoothed Weiszfeld iteration ("RFA": Pillutla, Kakade, Harchaoui,
// "Robust Aggregation for Federated Learning", IEEE TSP 2022) and centered clipping
// (Karimireddy, He, Jaggi, "Learning from History for Byzantine Robust Optimization", ICML
// 2021).  The reference repository has neither; the definitions live in include/fedhip.h and
// DESIGN.md §5.
//
// One iteration of either rule is  v_new = [v +] sum_k coef[k] * (x_k [- v])  followed by every
// client's squared distance to v_new, from which the next coefficients follow.  Built from the
// existing kernels that reads the [C][P] rows twice.  fh_center_iter reads them once: what
// ||x_k - v_new||^2 needs of coordinate j is column j and the coefficients, so a thread keeps
// the C values of its V columns in registers (the layout of rowslots.h: NP slots, a power of
// two, every register-array index a compile-time constant), forms out[j], stores it and
// adds (double)fl32(x_kj - out_j)^2 to its C fp64 accumulators.  HBM-bound: (C+1)*P floats read
// in DELTA, C*P in MEAN, P written.  At the end of its columns a wave folds its 64 x NP
// accumulators with a halving butterfly (NP - 1 exchanges, not 6*NP), the workgroup's four
// waves are added in wave order, and the partial goes to the workspace; a second small launch
// adds the workgroups' partials in a fixed order.  No atomics: the bits are a function of C, P
// and the alignments only.  Every fp32 operation is one rounded operation (the TU is built with
// -ffp-contract=off, no fmaf here); denormals are kept.
//
// fh_center_coef turns the distances into the next coefficients in fp64, one 64-thread launch.
#include <cmath>

#include "rowslots.h"

namespace fh {

constexpr int CI_MAXC = 64;

// One thread: V consecutive columns starting at begin + (tile*256 + tid)*V, tiles blockIdx.x,
// blockIdx.x + gridDim.x, ...  V > 1 needs 4*V-byte aligned rows / center / out (the host
// checks); V == 1 is the scalar path (any stride, any alignment, the tail).  center and out
// carry no __restrict__: they may be the same buffer, and every thread reads all it needs of a
// coordinate before it stores that coordinate.  part[k * nparts + part0 + blockIdx.x].
template <int NP, int V, int MODE>
__global__ void __launch_bounds__(256)
center_iter_kernel(const float* __restrict__ rows, int64_t row_stride,
                   const int32_t* __restrict__ row_index, const float* __restrict__ coef, int C,
                   int64_t begin, int64_t units, const float* center, float* out,
                   double* __restrict__ part, int nparts, int part0) {
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
        vec_t gv;
        if (MODE == FH_CENTER_DELTA) gv = *reinterpret_cast<const vec_t*>(center + col0 + lane_off);
        float res[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float g = MODE == FH_CENTER_DELTA ? reinterpret_cast<const float*>(&gv)[v] : 0.f;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                if (k < C) {
                    const float c = coef[k];
                    if (c != 0.0f) {  // +-0: the row is skipped, whatever it holds (wave-uniform)
                        const float x = reinterpret_cast<const float*>(&raw[k])[v];
                        const float d = MODE == FH_CENTER_DELTA ? (x - g) : x;
                        const float t = c * d;
                        acc = acc + t;
                    }
                }
            }
            res[v] = canon_nan(MODE == FH_CENTER_DELTA ? (g + acc) : acc);
        }
        *reinterpret_cast<vec_t*>(out + col0 + lane_off) = *reinterpret_cast<const vec_t*>(res);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            if (k < C) {
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const float d = reinterpret_cast<const float*>(&raw[k])[v] - res[v];
                    // (double)d * (double)d is exact in fp64 (48 significant bits), so the
                    // fused form rounds exactly once, as multiply-then-add would
                    sq[k] = fma((double)d, (double)d, sq[k]);
                }
            }
        }
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

// One wave per client, in part_sum's order (rowslots.h).  Written out: with the workgroup-uniform
// k the helper compiles to other address arithmetic than this loop (same sums, other machine
// code); whoever changes one order changes both.
__global__ void __launch_bounds__(64)
center_sqdist_finish_kernel(const double* __restrict__ part, int nparts,
                            double* __restrict__ sqdist) {
    const int k = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < nparts; b += 64) s += part[(int64_t)k * nparts + b];
    s = wave_sum(s);
    if (threadIdx.x == 0) sqdist[k] = s;
}

// 16-B columns up to 16 slots, 8-B at 32, one column at 64: the values and the fp64 accumulators
// stay in registers.
static constexpr int ci_vec(int NP) { return NP <= 16 ? 4 : (NP == 32 ? 2 : 1); }

template <int NP, int V>
static int ci_launch(int mode, const float* rows, int64_t row_stride, const int32_t* row_index,
                     const float* coef, int C, int64_t begin, int64_t units, const float* center,
                     float* out, double* part, int nparts, int part0, hipStream_t st) {
    const int grid = slots_grid(units, NP);
    if (mode == FH_CENTER_MEAN) {
        FH_LAUNCH((center_iter_kernel<NP, V, FH_CENTER_MEAN>), dim3(grid), dim3(256), 0, st, rows,
                  row_stride, row_index, coef, C, begin, units, center, out, part, nparts, part0);
    } else {
        FH_LAUNCH((center_iter_kernel<NP, V, FH_CENTER_DELTA>), dim3(grid), dim3(256), 0, st, rows,
                  row_stride, row_index, coef, C, begin, units, center, out, part, nparts, part0);
    }
    FH_LAUNCH_CHECK("center_iter");
    return FH_OK;
}

// ---- coefficients --------------------------------------------------------------------------
// One block of 64 threads, thread k = client k; the sums are thread 0's, left to right.
__global__ void __launch_bounds__(64)
center_coef_kernel(const double* __restrict__ sqdist, const double* __restrict__ alpha, int C,
                   int rule, double param, float* __restrict__ coef, double* __restrict__ state) {
    __shared__ double b[CI_MAXC], obj[CI_MAXC];
    __shared__ int live[CI_MAXC];
    __shared__ double total;
    const int k = threadIdx.x;
    double bk = 0.0;
    float ck = 0.f;
    if (k < C) {
        const double s = sqdist[k], a = alpha[k];
        const double d = sqrt(s);
        const bool lv = isfinite(s) && a > 0.0;
        if (rule == FH_CENTER_GEOMED) {
            bk = lv ? a / fmax(param, d) : 0.0;
        } else {
            ck = lv ? (float)(a * (d > param ? param / d : 1.0)) : 0.f;
            bk = (double)ck;
        }
        b[k] = bk;
        obj[k] = lv ? a * d : 0.0;
        live[k] = lv ? 1 : 0;
    }
    __syncthreads();
    if (k == 0) {
        double B = b[0], o = obj[0];  // a client that is not live adds +0 to both
        int n = live[0];
        for (int i = 1; i < C; ++i) {
            B = B + b[i];
            o = o + obj[i];
            n += live[i];
        }
        total = B;
        state[0] = (double)n;
        state[1] = o;
        state[2] = B;
        state[3] = param;
    }
    __syncthreads();
    if (k < C) {
        if (rule == FH_CENTER_GEOMED) {
            const double B = total;
            ck = (B == 0.0) ? 0.f : (float)(bk / B);
        }
        coef[k] = ck;
    }
}

}  // namespace fh

using namespace fh;

extern "C" size_t fh_center_iter_workspace(int32_t num_clients, int64_t P) {
    if (num_clients < 1 || num_clients > CI_MAXC || P <= 0) return 0;
    const int NP = slots_np(num_clients);
    return (size_t)num_clients * (size_t)slots_parts_max(NP, ci_vec(NP), P) * sizeof(double);
}

extern "C" int fh_center_iter(const float* rows, int64_t row_stride, const int32_t* row_index,
                              const float* coef, int32_t num_clients, int64_t P,
                              const float* center, int32_t mode, float* out, void* workspace,
                              size_t ws_bytes, double* sqdist, void* stream) {
    const int C = num_clients;
    FH_REQUIRE(mode == FH_CENTER_MEAN || mode == FH_CENTER_DELTA,
               "center_iter: mode=%d outside [0, 1]", mode);
    FH_REQUIRE(C >= 1 && C <= CI_MAXC, "center_iter: num_clients=%d outside [1, 64]", C);
    FH_REQUIRE(P >= 0 && row_stride >= 0, "center_iter: bad sizes P=%lld row_stride=%lld",
               (long long)P, (long long)row_stride);
    FH_REQUIRE(sqdist, "center_iter: null pointer");
    hipStream_t st = as_stream(stream);
    int nparts = 0;
    double* part = static_cast<double*>(workspace);
    if (P > 0) {
        FH_REQUIRE(rows && coef && out && (center || mode == FH_CENTER_MEAN),
                   "center_iter: null pointer");
        const size_t need = fh_center_iter_workspace(C, P);
        FH_REQUIRE(workspace && ws_bytes >= need,
                   "center_iter: workspace of %zu bytes, %zu needed", ws_bytes, need);
        const int NP = slots_np(C);
        const bool vec_ok = (row_stride % 4 == 0) && aligned16(rows, out) &&
                            (mode == FH_CENTER_MEAN || aligned16(center));
        const SlotsPlan plan = slots_plan(NP, ci_vec(NP), vec_ok, P);
        nparts = plan.nparts;
        const int rc = slots_dispatch<CI_MAXC, ci_vec>(
            NP, plan, P, [&](auto np, auto v, int64_t begin, int64_t units, int part0) {
                return ci_launch<decltype(np)::value, decltype(v)::value>(
                    mode, rows, row_stride, row_index, coef, C, begin, units, center, out, part,
                    nparts, part0, st);
            });
        if (rc != FH_OK) return rc;
    }
    FH_LAUNCH(center_sqdist_finish_kernel, dim3(C), dim3(64), 0, st,
              static_cast<const double*>(workspace), nparts, sqdist);
    FH_LAUNCH_CHECK("center_sqdist_finish");
    return FH_OK;
}

extern "C" int fh_center_coef(const double* sqdist, const double* alpha, int32_t num_clients,
                              int32_t rule, double param, float* coef, double* state,
                              void* stream) {
    FH_REQUIRE(rule == FH_CENTER_GEOMED || rule == FH_CENTER_CCLIP,
               "center_coef: rule=%d outside [0, 1]", rule);
    FH_REQUIRE(num_clients >= 1 && num_clients <= CI_MAXC,
               "center_coef: num_clients=%d outside [1, 64]", num_clients);
    FH_REQUIRE(std::isfinite(param) && param > 0.0,
               "center_coef: %s=%g must be finite and positive",
               rule == FH_CENTER_GEOMED ? "nu" : "tau", param);
    FH_REQUIRE(sqdist && alpha && coef && state, "center_coef: null pointer");
    FH_LAUNCH(center_coef_kernel, dim3(1), dim3(64), 0, as_stream(stream), sqdist, alpha,
              (int)num_clients, (int)rule, param, coef, state);
    FH_LAUNCH_CHECK("center_coef");
    return FH_OK;
}
