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
// fltrust_stats_kernel has qfedavg_main_kernel's layout (qfedavg.hip): a thread keeps the C
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

#include "fh_common.h"

namespace fh {

// row_index == NULL reads this instead: one code path, no branch around the index load
__device__ const int32_t flt_identity[64] = {
    0,  1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21,
    22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43,
    44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63};

template <int V> struct FltVec;
template <> struct FltVec<4> { using type = float4; };
template <> struct FltVec<2> { using type = float2; };
template <> struct FltVec<1> { using type = float; };

constexpr int FLT_MAXC = 64;
constexpr int FLT_MAXNP = 32;  // slots of one stats launch; 33..64 clients take two launches
constexpr int FLT_COEF_WAVES = 16;
constexpr size_t FLT_HEAD_BYTES = FLT_MAXC * sizeof(double);  // sqdist_after, workspace front

// Sum a[k] over the 64 lanes for every k < NP: center.hip's ci_wave_fold.  Stage t pairs lane l
// with l ^ (32 >> t): the lane with that bit clear keeps the lower half of the live slots, the
// other the upper half, each adds what its partner held of the half it keeps.  After log2(NP)
// stages a lane holds one slot, summed over 2^stages lanes; the remaining lane bits are a plain
// butterfly.  Returns that slot's wave total; *slot is its k.  A fixed order of additions.
template <int H, int O, int NP>
__device__ __forceinline__ void flt_fold_stage(double (&a)[NP], int lane, int& k) {
    if constexpr (H >= 1) {
        const bool upper = (lane & O) != 0;
#pragma unroll
        for (int i = 0; i < H; ++i) {
            const double send = upper ? a[i] : a[i + H];
            const double keep = upper ? a[i + H] : a[i];
            a[i] = keep + __shfl_xor(send, O, 64);
        }
        if (upper) k += H;
        flt_fold_stage<H / 2, O / 2, NP>(a, lane, k);
    }
}

template <int NP>
__device__ __forceinline__ double flt_wave_fold(double (&a)[NP], int lane, int* slot) {
    int k = 0;
    flt_fold_stage<NP / 2, 32, NP>(a, lane, k);
    double s = a[0];
#pragma unroll
    for (int o = 32 / NP; o >= 1; o /= 2) s += __shfl_xor(s, o, 64);
    *slot = k;
    return s;
}

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
    using vec_t = typename FltVec<V>::type;
    __shared__ double red[4][2 * NP + 1];
    const int32_t* ip = (row_index ? row_index : flt_identity) + k0;
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
        // All NP + 2 loads are issued before the first use, in straight-line code.  Slots past
        // C re-read row C-1 (a cache hit, no branch) and are never used.
        vec_t raw[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int64_t r = ip[k < C ? k : C - 1];
            raw[k] = *reinterpret_cast<const vec_t*>(rows + r * row_stride + col0 + lane_off);
        }
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
    int slot;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const double s = flt_wave_fold<NP>(sq, lane, &slot);
    const double t = flt_wave_fold<NP>(dot, lane, &slot);
    sq0 = wave_sum(sq0);
    if ((lane & (63 >> (31 - __builtin_clz(NP)))) == 0) {
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
            const double v = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];  // wave order
            const int out_slot = i == 2 * NP ? 2 * Ctot : (i < NP ? k0 + k : Ctot + k0 + k);
            part[(int64_t)out_slot * nparts + part0 + blockIdx.x] = v;
        }
    }
}

// One workgroup of 16 waves.  Wave w takes slots w, w + 16, ... of the 2*C + 1: lane i adds
// partials i, i + 64, ... in order, then the butterfly (qfedavg_den_kernel's order).  Thread 0
// then evaluates the fp64 lines of the contract, left to right, every operation on its own.
__global__ void __launch_bounds__(64 * FLT_COEF_WAVES)
fltrust_coef_kernel(const double* __restrict__ part, int nparts, int C, float* __restrict__ coef,
                    double* __restrict__ trust, double* __restrict__ stats,
                    double* __restrict__ state) {
    __shared__ double st[2 * FLT_MAXC + 1];
    __shared__ double ts_s[FLT_MAXC], nk_s[FLT_MAXC];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int i = wid; i < 2 * C + 1; i += FLT_COEF_WAVES) {
        double s = 0.0;
        for (int p = lane; p < nparts; p += 64) s += part[(int64_t)i * nparts + p];
        s = wave_sum(s);
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

// Workgroups of a stats launch over `units` threads' worth of columns: at most `cap`, every one
// with the same number of tiles (but the last ones).  A function of units and NP alone.
static inline int flt_np(int C) {
    int NP = 2;
    while (NP < C) NP *= 2;
    return NP;
}
// 2*NP + 1 fp64 accumulators beside the NP*V values: 16-B columns up to 8 slots, 8-B at 16, one
// column at 32 (DESIGN.md §5 has the register counts)
static inline int flt_vec(int NP) { return NP <= 8 ? 4 : (NP == 16 ? 2 : 1); }
static inline int flt_grid(int64_t units, int NP) {
    if (units <= 0) return 0;
    const int64_t cap = NP >= 32 ? 512 : (NP == 16 ? 1024 : 2048);
    const int64_t tiles = ceil_div(units, 256);
    return (int)ceil_div(tiles, ceil_div(tiles, cap));
}
static inline int flt_parts_vec(int NP, int64_t P) {
    const int V = flt_vec(NP);
    if (V == 1) return flt_grid(P, NP);
    const int64_t vecP = P / 4 * 4;
    return flt_grid(vecP / V, NP) + flt_grid(P - vecP, NP);
}
static inline int flt_parts(int C, int64_t P) {
    const int NP = flt_np(std::min(C, FLT_MAXNP));
    return std::max(flt_parts_vec(NP, P), flt_grid(P, NP));
}
static inline size_t flt_keep_bytes(int64_t P) {
    return ((size_t)P * sizeof(float) + 15) / 16 * 16;
}

template <int NP, int V>
static int flt_launch(const float* rows, int64_t row_stride, const int32_t* row_index, int C,
                      int k0, int Ctot, int64_t begin, int64_t units, const float* root,
                      const float* global, double* part, int nparts, int part0, hipStream_t st) {
    const int grid = flt_grid(units, NP);
    FH_LAUNCH((fltrust_stats_kernel<NP, V>), dim3(grid), dim3(256), 0, st, rows, row_stride,
              row_index, C, k0, Ctot, begin, units, root, global, part, nparts, part0);
    FH_LAUNCH_CHECK("fltrust_stats");
    return FH_OK;
}

// The stats of clients k0 .. k0 + C of Ctot, NP = flt_np(C) slots; vecP columns go through the
// vector instance (0: none), the rest through the scalar one.
static int flt_stats(const float* rows, int64_t row_stride, const int32_t* row_index, int C,
                     int k0, int Ctot, int NP, int64_t P, int64_t vecP, const float* root,
                     const float* global, double* part, int nparts, hipStream_t st) {
    const int vparts = vecP ? flt_grid(vecP / flt_vec(NP), NP) : 0;
    int rc = FH_OK;
#define FH_FLT_CASE(np, v)                                                                      \
    case np:                                                                                    \
        if (vecP)                                                                               \
            rc = flt_launch<np, v>(rows, row_stride, row_index, C, k0, Ctot, 0, vecP / v, root, \
                                   global, part, nparts, 0, st);                                \
        if (rc == FH_OK && vecP < P)                                                            \
            rc = flt_launch<np, 1>(rows, row_stride, row_index, C, k0, Ctot, vecP, P - vecP,    \
                                   root, global, part, nparts, vparts, st);                     \
        break;
    switch (NP) {
        FH_FLT_CASE(2, 4)
        FH_FLT_CASE(4, 4)
        FH_FLT_CASE(8, 4)
        FH_FLT_CASE(16, 2)
        default:
            rc = flt_launch<32, 1>(rows, row_stride, row_index, C, k0, Ctot, 0, P, root, global,
                                   part, nparts, 0, st);
    }
#undef FH_FLT_CASE
    return rc;
}

}  // namespace fh

using namespace fh;

// [sqdist_after: 64 doubles][g kept for the all-zero case: P floats, padded to 16 bytes]
// [partials: the larger of the stats pass's (2C+1) * parts doubles and fh_center_iter's]
extern "C" size_t fh_fltrust_workspace(int32_t num_clients, int64_t P) {
    if (num_clients < 1 || num_clients > FLT_MAXC || P <= 0) return 0;
    const size_t mine = (size_t)(2 * num_clients + 1) * (size_t)flt_parts(num_clients, P) *
                        sizeof(double);
    return FLT_HEAD_BYTES + flt_keep_bytes(P) +
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
                                         flt_keep_bytes(P));
        auto al16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
        const bool vec_ok = (row_stride % 4 == 0) && al16(rows) && al16(root) && al16(global);
        // Up to 32 clients one launch; 33..64 two launches over the halves of the index list,
        // both with the 32-slot instance (the 64-slot one would not fit the register file):
        // g and the root row are read twice.  Every launch has the same grid, so the partials
        // of a client sit at the same places whichever launch wrote them.
        const int C0 = std::min(C, FLT_MAXNP);
        const int NP = flt_np(C0);
        const int64_t vecP = (vec_ok && flt_vec(NP) > 1) ? P / 4 * 4 : 0;
        nparts = vecP ? flt_parts_vec(NP, P) : flt_grid(P, NP);
        int rc = flt_stats(rows, row_stride, row_index, C0, 0, C, NP, P, vecP, root, global, part,
                           nparts, st);
        if (rc == FH_OK && C > C0)
            rc = flt_stats(rows, row_stride, row_index, C - C0, C0, C, NP, P, vecP, root, global,
                           part, nparts, st);
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
        const size_t off = FLT_HEAD_BYTES + flt_keep_bytes(P);
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
