// robust.hip — Byzantine-robust aggregation of packed client rows: the coordinate-wise
// trimmed mean / median (Yin et al. 2018) and the pairwise squared distances that Krum /
// multi-Krum (Blanchard et al. 2017) score on.  The reference repository has no such rule;
// the definitions live in include/fedhip.h and DESIGN.md §5.
//
// fh_trimmed_mean_rows: HBM-bound like fedavg_vec4_kernel (reads C*P floats, writes P).  A
// thread loads the C values of its V columns into registers as 32-bit keys whose unsigned
// order is the total order  -Inf < ... < -0 < +0 < ... < +Inf < NaN, sorts them with a
// compile-time Batcher odd-even merge network on v_min_u32 / v_max_u32 (padded to NP slots,
// a power of two; pad slots hold a key above the NaN key), maps the kept keys back and adds
// them in ascending order.  Every register-array index is a compile-time constant after
// unrolling, so nothing lives in scratch.  No FMA (the TU is built with -ffp-contract=off).
//
// fh_pairwise_sqdist: each workgroup owns a chunk of coordinates, stages [C][64] tiles of it
// in LDS once (row pitch 65: lanes reading different rows at one column hit different banks,
// lanes reading the same row broadcast), thread p owns pairs p, p+256, ... and walks the
// columns; the rows are read from HBM once, not once per pair.  Partials go to the workspace
// and a second small launch adds them in chunk order: no atomics, same bits on every run.
#include "rowslots.h"

namespace fh {

// ---------------------------------------------------------------- trimmed mean / median
constexpr uint32_t TM_KEY_NAN = 0xFFC00000u;  // one key for every NaN, above key(+Inf) = 0xFF800000
constexpr uint32_t TM_KEY_PAD = 0xFFFFFFFFu;  // pad slots sort after everything

__device__ __forceinline__ uint32_t tm_key(float x) {
    const uint32_t b = __float_as_uint(x);
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return TM_KEY_NAN;
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ float tm_val(uint32_t k) {
    return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
}

// Batcher's odd-even merge sort of NP keys (NP a power of two), ascending.  All four loops
// have compile-time bounds once the outer ones are unrolled.
template <int NP>
__device__ __forceinline__ void tm_sort(uint32_t (&s)[NP]) {
#pragma unroll
    for (int p = 1; p < NP; p *= 2) {
#pragma unroll
        for (int k = p; k >= 1; k /= 2) {
#pragma unroll
            for (int j = k % p; j <= NP - 1 - k; j += 2 * k) {
#pragma unroll
                for (int i = 0; i <= (k - 1 < NP - j - k - 1 ? k - 1 : NP - j - k - 1); ++i) {
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                        const uint32_t a = s[i + j], b = s[i + j + k];
                        s[i + j] = min(a, b);
                        s[i + j + k] = max(a, b);
                    }
                }
            }
        }
    }
}

// One thread: V consecutive columns starting at begin + q*V.  V > 1 needs 4*V-byte aligned
// rows / out (the host checks); V == 1 is the scalar path (any stride, any alignment, tail).
template <int NP, int V>
__global__ void __launch_bounds__(256)
trimmed_mean_kernel(const float* __restrict__ rows, int64_t row_stride,
                    const int32_t* __restrict__ row_index, int C, int trim, int64_t begin,
                    int64_t units, float* __restrict__ out) {
    using vec_t = typename SlotVec<V>::type;
    const int hi = C - 1 - trim;
    const float denom = (float)(C - 2 * trim);
    const int32_t* ip = row_index ? row_index : slots_identity;
    const uint32_t lane_off = threadIdx.x * V;
    for (int64_t blk = blockIdx.x; blk * 256 < units; blk += gridDim.x) {
        if (blk * 256 + threadIdx.x >= units) break;  // only in the last block of columns
        const int64_t col0 = begin + blk * (256 * V);
        // slots_load, written out: the compiler shares this C - 1 with hi's, and through the
        // helper it would form hi another way.  Slots past C get the pad key below.
        vec_t raw[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int64_t r = ip[k < C ? k : C - 1];
            raw[k] = *reinterpret_cast<const vec_t*>(rows + r * row_stride + col0 + lane_off);
        }
        float res[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            uint32_t s[NP];
#pragma unroll
            for (int k = 0; k < NP; ++k)
                s[k] = k < C ? tm_key(reinterpret_cast<const float*>(&raw[k])[v]) : TM_KEY_PAD;
            tm_sort<NP>(s);
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const float x = tm_val(s[k]);
                if (k == trim) acc = x;
                else if (k > trim && k <= hi) acc = acc + x;
            }
            acc = acc / denom;
            res[v] = canon_nan(acc);
        }
        *reinterpret_cast<vec_t*>(out + col0 + lane_off) = *reinterpret_cast<const vec_t*>(res);
    }
}

// 16-B columns up to 16 slots, 8-B at 32, one column at 64: the keys stay in registers at >= 2
// waves per SIMD.
static constexpr int tm_vec(int NP) { return NP <= 16 ? 4 : (NP == 32 ? 2 : 1); }

template <int NP, int V>
static int tm_launch(const float* rows, int64_t row_stride, const int32_t* row_index, int C,
                     int trim, int64_t begin, int64_t units, float* out, hipStream_t st) {
    FH_LAUNCH((trimmed_mean_kernel<NP, V>), dim3(stream_grid(units)), dim3(256), 0, st, rows,
              row_stride, row_index, C, trim, begin, units, out);
    FH_LAUNCH_CHECK("trimmed_mean");
    return FH_OK;
}

// ---------------------------------------------------------------- pairwise distances
constexpr int PW_T = 64;            // columns per LDS tile
constexpr int PW_PITCH = PW_T + 1;  // row pitch in floats
constexpr int PW_MAXC = 64;
constexpr int PW_PP = 8;            // pairs per thread: ceil(64*63/2 / 256)
constexpr int64_t PW_GRID = 1024;   // target number of chunks

static inline int64_t pw_chunk(int64_t P) {  // columns per workgroup, a multiple of PW_T
    return std::max<int64_t>(PW_T, ceil_div(ceil_div(P, PW_GRID), PW_T) * PW_T);
}

// part[chunk][pair], pair (a < b) numbered row-major over the strict upper triangle.
__global__ void __launch_bounds__(256)
pairwise_partial_kernel(const float* __restrict__ rows, int64_t row_stride,
                        const int32_t* __restrict__ row_index, int C, int64_t P, int64_t chunk,
                        double* __restrict__ part) {
    __shared__ float tile[PW_MAXC * PW_PITCH];
    const int npairs = C * (C - 1) / 2;
    const int npp = (npairs + 255) / 256;  // uniform: pair slots in use per thread
    int ao[PW_PP], bo[PW_PP];
#pragma unroll
    for (int i = 0; i < PW_PP; ++i) {
        int p = threadIdx.x + 256 * i;
        int a = 0, b = 0;  // slots past the last pair compare row 0 with itself (adds +0)
        if (p < npairs) {
            while (p >= C - 1 - a) {
                p -= C - 1 - a;
                ++a;
            }
            b = a + 1 + p;
        }
        ao[i] = a * PW_PITCH;
        bo[i] = b * PW_PITCH;
    }
    double acc[PW_PP];
#pragma unroll
    for (int i = 0; i < PW_PP; ++i) acc[i] = 0.0;
    const int64_t j0 = blockIdx.x * chunk, j1 = std::min<int64_t>(P, j0 + chunk);
    for (int64_t base = j0; base < j1; base += PW_T) {
        const int n = (int)std::min<int64_t>(PW_T, j1 - base);
        for (int e = threadIdx.x; e < C * PW_T; e += 256) {
            const int r = e / PW_T, c = e % PW_T;
            const int64_t src = row_index ? row_index[r] : r;
            // columns past the end hold 0 in every row: their differences add +0
            tile[r * PW_PITCH + c] = c < n ? rows[src * row_stride + base + c] : 0.f;
        }
        __syncthreads();
        for (int c = 0; c < PW_T; ++c) {
#pragma unroll
            for (int i = 0; i < PW_PP; ++i) {
                if (i < npp) {
                    const float d = tile[ao[i] + c] - tile[bo[i] + c];  // one rounded fp32 sub
                    // (double)d * (double)d is exact in fp64 (48 significant bits), so the
                    // fused form rounds exactly once, as multiply-then-add would
                    acc[i] = fma((double)d, (double)d, acc[i]);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < PW_PP; ++i) {
        const int p = threadIdx.x + 256 * i;
        if (p < npairs) part[(int64_t)blockIdx.x * npairs + p] = acc[i];
    }
}

// One thread per (a, b), a <= b: partials added in chunk order; both halves and the diagonal.
__global__ void __launch_bounds__(256)
pairwise_reduce_kernel(const double* __restrict__ part, int C, int nchunks,
                       double* __restrict__ dist) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= C * C) return;
    const int a = t / C, b = t % C;
    if (a > b) return;
    if (a == b) {
        dist[t] = 0.0;
        return;
    }
    const int npairs = C * (C - 1) / 2;
    const int p = a * (C - 1) - a * (a - 1) / 2 + (b - a - 1);
    double s = 0.0;
    for (int ch = 0; ch < nchunks; ++ch) s += part[(int64_t)ch * npairs + p];
    dist[a * C + b] = s;
    dist[b * C + a] = s;
}

}  // namespace fh

using namespace fh;

extern "C" int fh_trimmed_mean_rows(const float* rows, int64_t row_stride,
                                    const int32_t* row_index, int32_t num_clients, int32_t trim,
                                    int64_t P, float* out, void* stream) {
    const int C = num_clients;
    FH_REQUIRE(C >= 1 && C <= 64, "trimmed_mean: num_clients=%d outside [1, 64]", C);
    FH_REQUIRE(trim >= 0 && 2 * (int64_t)trim < C,
               "trimmed_mean: trim=%d per side leaves nothing of %d clients (need 0 <= 2*trim < C)",
               trim, C);
    FH_REQUIRE(P >= 0 && row_stride >= 0, "trimmed_mean: bad sizes P=%lld row_stride=%lld",
               (long long)P, (long long)row_stride);
    if (P == 0) return FH_OK;
    FH_REQUIRE(rows && out, "trimmed_mean: null pointer");
    hipStream_t st = as_stream(stream);
    const int NP = slots_np(C);
    const bool vec_ok = (row_stride % 4 == 0) && aligned16(rows, out);
    // no reduction over columns here: the plan's partial counts go unused
    return slots_dispatch<64, tm_vec>(
        NP, slots_plan(NP, tm_vec(NP), vec_ok, P), P,
        [&](auto np, auto v, int64_t begin, int64_t units, int) {
            return tm_launch<decltype(np)::value, decltype(v)::value>(
                rows, row_stride, row_index, C, trim, begin, units, out, st);
        });
}

extern "C" size_t fh_pairwise_sqdist_workspace(int32_t num_clients, int64_t P) {
    if (num_clients < 2 || num_clients > PW_MAXC || P <= 0) return 0;
    const int64_t npairs = (int64_t)num_clients * (num_clients - 1) / 2;
    return (size_t)(ceil_div(P, pw_chunk(P)) * npairs) * sizeof(double);
}

extern "C" int fh_pairwise_sqdist(const float* rows, int64_t row_stride, const int32_t* row_index,
                                  int32_t num_clients, int64_t P, void* workspace,
                                  size_t ws_bytes, double* dist, void* stream) {
    const int C = num_clients;
    FH_REQUIRE(C >= 2 && C <= PW_MAXC, "pairwise_sqdist: num_clients=%d outside [2, 64]", C);
    FH_REQUIRE(P >= 0 && row_stride >= 0, "pairwise_sqdist: bad sizes P=%lld row_stride=%lld",
               (long long)P, (long long)row_stride);
    FH_REQUIRE(dist, "pairwise_sqdist: null pointer");
    hipStream_t st = as_stream(stream);
    int nchunks = 0;
    if (P > 0) {
        FH_REQUIRE(rows, "pairwise_sqdist: null pointer");
        const size_t need = fh_pairwise_sqdist_workspace(C, P);
        FH_REQUIRE(workspace && ws_bytes >= need,
                   "pairwise_sqdist: workspace of %zu bytes, %zu needed", ws_bytes, need);
        const int64_t chunk = pw_chunk(P);
        nchunks = (int)ceil_div(P, chunk);
        FH_LAUNCH(pairwise_partial_kernel, dim3(nchunks), dim3(256), 0, st, rows, row_stride,
                  row_index, C, P, chunk, static_cast<double*>(workspace));
        FH_LAUNCH_CHECK("pairwise_partial");
    }
    FH_LAUNCH(pairwise_reduce_kernel, dim3((unsigned)ceil_div(C * C, 256)), dim3(256), 0, st,
              static_cast<const double*>(workspace), C, nchunks, dist);
    FH_LAUNCH_CHECK("pairwise_reduce");
    return FH_OK;
}
