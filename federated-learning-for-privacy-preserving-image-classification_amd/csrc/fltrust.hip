// fltrust.hip — FLTrust, trust-scored aggregation against a server root update (Cao, Fang, Liu,
// Gong, "FLTrust: Byzantine-robust Federated Learning via Trust Bootstrapping", NDSS 2021,
// Algorithm 2).  The reference repository has only the sample-weighted FedAvg; the definitions
// live in include/fedhip.h and DESIGN.md §5.
//
// With the global model g the round started from, the server's own trained row r and client k's
// trained row x_k, the deltas are d0 = r - g and d_k = x_k - g.  A client's trust score is the
// cosine of the angle between d_k and d0, clipped to [0, 1]; its delta is rescaled to ||d0|| and
// the server sets
//     g_new = g + sum_k c_k * d_k,   c_k = ts_k * (||d0|| / ||d_k||) / sum_i ts_i.
// The scores need every client's dot product with d0 and its squared norm.  No other kernel of
// the library forms a dot product against a reference direction, so the first pass is new:
// fltrust_stats_kernel has the register-slot layout of rowslots.h: a thread keeps the C
// values of its V columns in registers (NP slots, a power of two, every register-array index a
// compile-time constant) next to g and r, turns them into the fp32 differences and adds
// (double)d_kj^2, (double)d_kj*(double)d0_j and (double)d0_j^2 to 2*NP + 1 fp64 accumulators.
// HBM-bound: (C+2)*P floats read, nothing of size P written.  A wave folds its accumulators with
// the halving butterfly, the workgroup's four waves are added in wave order and the partials go
// to the workspace.  A second, one-workgroup launch adds the workgroups' partials in a fixed
// order and evaluates the scores and the coefficients in fp64, left to right; they stay on the
// device.  FH_FLT_STEP then applies the coefficients with fh_center_iter in FH_CENTER_DELTA mode
// (center.hip): the weighted delta sum is not written a third time.  No atomics, no allocation,
// no host synchronisation: the bits are a function of C, P and the alignments only.  Every fp32
// operation is one rounded operation (the TU is built with -ffp-contract=off, no fmaf here);
// denormals are kept.
#include <cmath>

#include "rowslots.h"

namespace fh {

constexpr int FLT_MAXC = 64;
constexpr int FLT_MAXNP = 32;  // slots of one stats launch; 33..64 clients take two launches
constexpr int FLT_COEF_WAVES = 16;
constexpr size_t FLT_HEAD_BYTES = FLT_MAXC * sizeof(double);  // sqdist_after, workspace front

// One thread: V consecutive columns starting at begin + (tile*256 + tid)*V, tiles blockIdx.x,
// blockIdx.x + gridDim.x, ...  V > 1 needs 4*V-byte aligned rows / root / global (the host
// checks); V == 1 is the scalar path (any stride, any alignment, the tail).  The launch covers
// the C clients row_index[k0 .. k0 + C) of the call's Ctot.  Partials, [2*Ctot + 1][nparts]:
// slot k0 + k is sq_k, slot Ctot + k0 + k is dot_k, slot 2*Ctot is sq0 (the k0 == 0 launch
// writes it); part[slot * nparts + part0 + blockIdx.x].
template <int NP, int V>
__global__ void __launch_bounds__(256)
fltrust_stats_kernel(const float* __restrict__ rows, int64_t row_stride,
                     const int32_t* __restrict__ row_index, int C, int k0, int Ctot,
                     int64_t begin, int64_t units, const float* __restrict__ root,
                     const float* __restrict__ global, double* __restrict__ part, int nparts,
                     int part0) {
    using vec_t = typename SlotVec<V>::type;
    __shared__ double red[4][2 * NP + 1];
    const int32_t* ip = (row_index ? row_index : slots_identity) + k0;
    const uint32_t lane_off = threadIdx.x * V;
    double sq[NP], dot[NP];
    double sq0 = 0.0;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        sq[k] = 0.0;
        dot[k] = 0.0;
    }
    for (int64_t blk = blockIdx.x; blk * 256 < units; blk += gridDim.x) {
        if (blk * 256 + threadIdx.x >= units) break;  // only in the last tile of columns
        const int64_t col0 = begin + blk * (256 * V);
        // the NP + 2 loads are issued before the first use
        vec_t raw[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k)
            raw[k] = slots_load<V>(rows, row_stride, ip, C, k, col0, lane_off);
        const vec_t gv = *reinterpret_cast<const vec_t*>(global + col0 + lane_off);
        const vec_t rv = *reinterpret_cast<const vec_t*>(root + col0 + lane_off);
        double d0[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float d = reinterpret_cast<const float*>(&rv)[v] -
                            reinterpret_cast<const float*>(&gv)[v];
            d0[v] = (double)d;
            // exact products (48 significant bits): the fused form rounds once, as
            // multiply-then-add would (the argument of qfedavg.hip's squares)
            sq0 = fma(d0[v], d0[v], sq0);
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            if (k < C) {
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const float d = reinterpret_cast<const float*>(&raw[k])[v] -
                                    reinterpret_cast<const float*>(&gv)[v];
                    sq[k] = fma((double)d, (double)d, sq[k]);
                    dot[k] = fma((double)d, d0[v], dot[k]);
                }
            }
        }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int slot;
    const double s = slots_wave_fold<NP>(sq, lane, &slot);
    const double t = slots_wave_fold<NP>(dot, lane, &slot);
    sq0 = wave_sum(sq0);
    if (slots_owner<NP>(lane)) {
        red[wid][slot] = s;
        red[wid][NP + slot] = t;
    }
    if (lane == 0) red[wid][2 * NP] = sq0;
    __syncthreads();
    const int i = threadIdx.x;
    if (i < 2 * NP + 1) {
        const int k = i < NP ? i : i - NP;  // i == 2*NP: the root's own slot
        const bool mine = i == 2 * NP ? k0 == 0 : k < C;
        if (mine) {
            const double v = slots_block_sum(red, i);
            const int out_slot = i == 2 * NP ? 2 * Ctot : (i < NP ? k0 + k : Ctot + k0 + k);
            part[(int64_t)out_slot * nparts + part0 + blockIdx.x] = v;
        }
    }
}

// One workgroup of 16 waves.  Wave w finishes slots w, w + 16, ... of the 2*C + 1 (part_sum).
// Thread 0 then evaluates the fp64 lines of the contract, left to right, every operation on its
// own.
__global__ void __launch_bounds__(64 * FLT_COEF_WAVES)
fltrust_coef_kernel(const double* __restrict__ part, int nparts, int C, float* __restrict__ coef,
                    double* __restrict__ trust, double* __restrict__ stats,
                    double* __restrict__ state) {
    __shared__ double st[2 * FLT_MAXC + 1];
    __shared__ double ts_s[FLT_MAXC], nk_s[FLT_MAXC];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int i = wid; i < 2 * C + 1; i += FLT_COEF_WAVES) {
        const double s = part_sum(part, i, nparts, lane);
        if (lane == 0) {
            st[i] = s;
            stats[i] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double sq0 = st[2 * C];
        const double n0 = sqrt(sq0);
        const bool root_ok = isfinite(sq0) && sq0 > 0.0;
        double S = 0.0;
        int live = 0, trusted = 0;
        for (int k = 0; k < C; ++k) {
            const double sq = st[k], dot = st[C + k];
            double ts = 0.0, nk = 0.0;  // a client that is not live has ts = 0
            if (isfinite(sq) && sq > 0.0 && isfinite(dot)) {
                ++live;
                nk = sqrt(sq);
                const double den = nk * n0;
                const double q = dot / den;
                ts = q > 0.0 ? q : 0.0;  // max(0, q); a NaN quotient (zero root) gives 0
                ts = ts > 1.0 ? 1.0 : ts;
            }
            if (ts > 0.0) ++trusted;
            ts_s[k] = ts;
            nk_s[k] = nk;
            trust[k] = ts;
            S = k == 0 ? ts : S + ts;
        }
        const bool ok = root_ok && isfinite(S) && S > 0.0;
        for (int k = 0; k < C; ++k) {
            float c = 0.f;
            if (ok && ts_s[k] > 0.0) {
                const double scale = n0 / nk_s[k];
                const double w = ts_s[k] * scale;
                c = (float)(w / S);
            }
            coef[k] = c;
        }
        state[0] = S;
        state[1] = (double)live;
        state[2] = (double)trusted;
        state[3] = n0;
    }
}

// dst = src, bit for bit, when every coefficient is zero; else nothing.  fh_center_iter's DELTA
// step stores canon(g + +0) for an all-zero coefficient vector, which turns -0 into +0 and a NaN
// payload into the one quiet NaN; the contract wants g itself.  One launch before the step
// keeps g in the workspace, one after it puts g into out (which may BE global), and in every
// other call both return at once.
__global__ void __launch_bounds__(256)
fltrust_keep_global_kernel(const float* __restrict__ coef, int C, const uint32_t* src,
                           uint32_t* dst, int64_t P) {
    const int lane = threadIdx.x & 63;
    const bool nz = lane < C && coef[lane] != 0.0f;
    if (__ballot(nz) != 0ull) return;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < P;
         j += (int64_t)gridDim.x * blockDim.x)
        dst[j] = src[j];
}

// 2*NP + 1 fp64 accumulators beside the NP*V values: 16-B columns up to 8 slots, 8-B at 16, one
// column at 32 (DESIGN.md §5 has the register counts)
static constexpr int flt_vec(int NP) { return NP <= 8 ? 4 : (NP == 16 ? 2 : 1); }
static inline int flt_parts(int C, int64_t P) {
    const int NP = slots_np(std::min(C, FLT_MAXNP));
    return slots_parts_max(NP, flt_vec(NP), P);
}

template <int NP, int V>
static int flt_launch(const float* rows, int64_t row_stride, const int32_t* row_index, int C,
                      int k0, int Ctot, int64_t begin, int64_t units, const float* root,
                      const float* global, double* part, int nparts, int part0, hipStream_t st) {
    const int grid = slots_grid(units, NP);
    FH_LAUNCH((fltrust_stats_kernel<NP, V>), dim3(grid), dim3(256), 0, st, rows, row_stride,
              row_index, C, k0, Ctot, begin, units, root, global, part, nparts, part0);
    FH_LAUNCH_CHECK("fltrust_stats");
    return FH_OK;
}

}  // namespace fh

using namespace fh;

// [sqdist_after: 64 doubles][g kept for the all-zero case: P floats, padded to 16 bytes]
// [partials: the larger of the stats pass's (2C+1) * parts doubles and fh_center_iter's]
extern "C" size_t fh_fltrust_workspace(int32_t num_clients, int64_t P) {
    if (num_clients < 1 || num_clients > FLT_MAXC || P <= 0) return 0;
    const size_t mine = (size_t)(2 * num_clients + 1) * (size_t)flt_parts(num_clients, P) *
                        sizeof(double);
    return FLT_HEAD_BYTES + pad16_floats(P) +
           std::max(mine, fh_center_iter_workspace(num_clients, P));
}

extern "C" int fh_fltrust_rows(const float* rows, int64_t row_stride, const int32_t* row_index,
                               int32_t num_clients, int64_t P, const float* root,
                               const float* global, int32_t mode, float* out, void* workspace,
                               size_t ws_bytes, float* coef, double* trust, double* stats,
                               double* state, void* stream) {
    const int C = num_clients;
    FH_REQUIRE(mode == FH_FLT_SCORE || mode == FH_FLT_STEP, "fltrust: mode=%d outside [0, 1]",
               mode);
    FH_REQUIRE(C >= 1 && C <= FLT_MAXC, "fltrust: num_clients=%d outside [1, 64]", C);
    FH_REQUIRE(P >= 0 && row_stride >= 0, "fltrust: bad sizes P=%lld row_stride=%lld",
               (long long)P, (long long)row_stride);
    FH_REQUIRE(coef && trust && stats && state, "fltrust: null coef, trust, stats or state");
    hipStream_t st = as_stream(stream);
    int nparts = 0;
    double* part = nullptr;
    if (P > 0) {
        FH_REQUIRE(rows && root && global && (out || mode == FH_FLT_SCORE),
                   "fltrust: null pointer");
        const size_t need = fh_fltrust_workspace(C, P);
        FH_REQUIRE(workspace && ws_bytes >= need && reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
                   "fltrust: workspace of %zu bytes, %zu needed (8-byte aligned)", ws_bytes, need);
        part = reinterpret_cast<double*>(static_cast<char*>(workspace) + FLT_HEAD_BYTES +
                                         pad16_floats(P));
        const bool vec_ok = (row_stride % 4 == 0) && aligned16(rows, root, global);
        // Up to 32 clients one launch; 33..64 two launches over the halves of the index list,
        // both with the 32-slot instance (the 64-slot one would not fit the register file):
        // g and the root row are read twice.  Every launch has the same grid, so the partials
        // of a client sit at the same places whichever launch wrote them.
        const int C0 = std::min(C, FLT_MAXNP);
        const int NP = slots_np(C0);
        const SlotsPlan plan = slots_plan(NP, flt_vec(NP), vec_ok, P);
        nparts = plan.nparts;
        int rc = FH_OK;
        for (int k0 = 0; rc == FH_OK && k0 < C; k0 += C0)
            rc = slots_dispatch<FLT_MAXNP, flt_vec>(
                NP, plan, P, [&](auto np, auto v, int64_t begin, int64_t units, int part0) {
                    return flt_launch<decltype(np)::value, decltype(v)::value>(
                        rows, row_stride, row_index, std::min(C - k0, C0), k0, C, begin, units,
                        root, global, part, nparts, part0, st);
                });
        if (rc != FH_OK) return rc;
    }
    FH_LAUNCH(fltrust_coef_kernel, dim3(1), dim3(64 * FLT_COEF_WAVES), 0, st,
              static_cast<const double*>(part), nparts, C, coef, trust, stats, state);
    FH_LAUNCH_CHECK("fltrust_coef");
    if (mode == FH_FLT_STEP && P > 0) {
        double* sqdist_after = static_cast<double*>(workspace);
        uint32_t* keep = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + FLT_HEAD_BYTES);
        const int grid = (int)std::min<int64_t>(ceil_div(P, 256), 1024);
        FH_LAUNCH(fltrust_keep_global_kernel, dim3(grid), dim3(256), 0, st,
                  static_cast<const float*>(coef), C, reinterpret_cast<const uint32_t*>(global),
                  keep, P);
        FH_LAUNCH_CHECK("fltrust_keep_global");
        const size_t off = FLT_HEAD_BYTES + pad16_floats(P);
        const int rc = fh_center_iter(rows, row_stride, row_index, coef, C, P, global,
                                      FH_CENTER_DELTA, out, part, ws_bytes - off, sqdist_after,
                                      stream);
        if (rc != FH_OK) return rc;
        FH_LAUNCH(fltrust_keep_global_kernel, dim3(grid), dim3(256), 0, st,
                  static_cast<const float*>(coef), C, static_cast<const uint32_t*>(keep),
                  reinterpret_cast<uint32_t*>(out), P);
        FH_LAUNCH_CHECK("fltrust_keep_global");
    }
    return FH_OK;
}
