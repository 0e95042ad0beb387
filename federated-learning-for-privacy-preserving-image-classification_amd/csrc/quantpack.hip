// quantpack.hip — packed quantised updates: bit-packed codes and FedAvg from them.
// The quantiser's counterpart of sparse.hip; the definition lives in
// include/fedhip.h.
//
// Reference: QuantizationCompressor.compress ships one uint8 tensor per layer plus
// quantization_params {scale, zero_point} (src/shared/compression.py:138-172) and
// _dequantize_tensor (:230-244) rebuilds the dense tensor.  Here a client's payload is one code
// row: segment s starts at byte boff[s] (16-byte aligned) and holds its elements' codes cw bits
// each (cw = 1, 2, 4 or 8 for bits 1, 2, 3..4, 5..8), low bits first, next to scale / zp as
// fh_quantize_rows wrote them and passv for the segments it passed through.
//
//   fh_quant_pack_rows    one code per byte -> cw bits per code; a passed-through segment ships
//                         the sign bits of v and its first element.
//   fh_quant_validate     per (segment, client): codes below 2^bits, scale finite and >= 0.
//   fh_quant_unpack_rows  out = base + d,  d = fl32(fl32((float)code - (float)zp) * (float)scale).
//   fh_quant_fedavg       out = [out +] sum_k fl32(w_k) * fl32(base + d_k) without the dense rows.
//
// Work decomposition of pack, unpack and fedavg: every CHUNK-element chunk of the segment plan is
// cut into QP_SUBS pieces of QP_SUB elements, one workgroup each; a lane owns QP_RUN = 16
// consecutive elements, whose codes are one aligned load of 2 * cw bytes (16 bytes at cw = 8), so
// a wave reads 128 * cw consecutive bytes per client.  A piece starts QP_SUB * cw / 8 bytes into
// its segment: every load is aligned to its own size.  No LDS, no barrier, no atomics.
//
// fh_quant_fedavg keeps a lane's 16 accumulators and base values in registers and walks the
// clients in row_index order with the code loads of the next QP_PF clients in flight; a client's
// (float)scale, (float)zp and flag are uniform over the workgroup.  HBM traffic: cw/8 bytes per
// element and client, 8 per parameter.  The TU is built with -ffp-contract=off and has no fused
// multiply-add: every fp32 operation is rounded on its own.
#include "fh_common.h"

namespace fh {

static constexpr int QP_CHUNK = 8192;  // == fh_compress_chunk_elems() (checked at launch)
static constexpr int QP_THREADS = 256;
static constexpr int QP_RUN = 16;      // elements per lane
static constexpr int QP_SUB = QP_THREADS * QP_RUN;
static constexpr int QP_SUBS = QP_CHUNK / QP_SUB;
static constexpr int QP_PF = 4;        // clients whose codes are in flight per lane

__device__ __forceinline__ int qp_seg_of_chunk(const int32_t* __restrict__ chunk_offsets, int nseg,
                                               int chunk) {
    int lo = 0, hi = nseg - 1;  // largest s with chunk_offsets[s] <= chunk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (chunk_offsets[mid] <= chunk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One QP_SUB piece of a chunk: row elements [e0, e0 + len), segment-local indices from c0.
struct QpSub {
    int s, len;
    int64_t e0, c0;
};

__device__ __forceinline__ QpSub qp_sub(const int64_t* __restrict__ seg_offsets,
                                        const int32_t* __restrict__ chunk_offsets, int nseg,
                                        int block) {
    const int chunk = block / QP_SUBS;
    QpSub g;
    g.s = qp_seg_of_chunk(chunk_offsets, nseg, chunk);
    const int64_t s0 = seg_offsets[g.s], s1 = seg_offsets[g.s + 1];
    g.c0 = (int64_t)(chunk - chunk_offsets[g.s]) * QP_CHUNK + (int64_t)(block % QP_SUBS) * QP_SUB;
    g.e0 = s0 + g.c0;
    const int64_t e1 = min(g.e0 + (int64_t)QP_SUB, s1);
    g.len = e1 > g.e0 ? (int)(e1 - g.e0) : 0;
    return g;
}

// A lane's QP_RUN codes of CW bits: 2 * CW bytes in 32-bit words, low bits first.
template <int CW>
struct QpCodes {
    static constexpr int NW = CW >= 2 ? CW / 2 : 1;
    uint32_t w[NW];
};

template <int CW>
__device__ __forceinline__ uint32_t qp_code(const QpCodes<CW>& c, int u) {
    const int bit = u * CW;
    return (c.w[bit >> 5] >> (bit & 31)) & ((1u << CW) - 1u);
}

// The codes of a run of n elements at p (aligned to 2 * CW bytes).  A full run is one load; a
// short one reads its ceil(n * CW / 8) bytes one by one and nothing behind them.
template <int CW>
__device__ __forceinline__ QpCodes<CW> qp_load(const uint8_t* __restrict__ p, int n) {
    QpCodes<CW> c;
    if (n == QP_RUN) {
        if constexpr (CW == 8) {
            const uint4 v = *reinterpret_cast<const uint4*>(p);
            c.w[0] = v.x; c.w[1] = v.y; c.w[2] = v.z; c.w[3] = v.w;
        } else if constexpr (CW == 4) {
            const uint2 v = *reinterpret_cast<const uint2*>(p);
            c.w[0] = v.x; c.w[1] = v.y;
        } else if constexpr (CW == 2) {
            c.w[0] = *reinterpret_cast<const uint32_t*>(p);
        } else {
            c.w[0] = *reinterpret_cast<const uint16_t*>(p);
        }
        return c;
    }
#pragma unroll
    for (int q = 0; q < QpCodes<CW>::NW; ++q) c.w[q] = 0u;
    const int nb = (n * CW + 7) >> 3;
#pragma unroll
    for (int b = 0; b < 2 * CW; ++b)
        if (b < nb) c.w[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
    return c;
}

template <int CW>
__device__ __forceinline__ void qp_store(uint8_t* __restrict__ p, const QpCodes<CW>& c, int n) {
    if (n == QP_RUN) {
        if constexpr (CW == 8)
            *reinterpret_cast<uint4*>(p) = make_uint4(c.w[0], c.w[1], c.w[2], c.w[3]);
        else if constexpr (CW == 4)
            *reinterpret_cast<uint2*>(p) = make_uint2(c.w[0], c.w[1]);
        else if constexpr (CW == 2)
            *reinterpret_cast<uint32_t*>(p) = c.w[0];
        else
            *reinterpret_cast<uint16_t*>(p) = (uint16_t)c.w[0];
        return;
    }
    const int nb = (n * CW + 7) >> 3;
#pragma unroll
    for (int b = 0; b < 2 * CW; ++b)
        if (b < nb) p[b] = (uint8_t)(c.w[b >> 2] >> (8 * (b & 3)));
}

// One client's header of one segment, uniform over the workgroup.
struct QpHead {
    float fs, fzp;
    uint32_t mag;  // bit 31: the segment was passed through, d = the magnitude bits of passv (bits
                   // 0..30) under the code's bit 0 as sign
};

__device__ __forceinline__ QpHead qp_head(const double* __restrict__ scale,
                                          const int64_t* __restrict__ zp,
                                          const float* __restrict__ passv, int64_t at) {
    QpHead h;
    const int64_t z = zp[at];
    h.fs = (float)scale[at];
    h.fzp = (float)z;
    h.mag = (__float_as_uint(passv[at]) & 0x7FFFFFFFu) | (z == INT64_MIN ? 0x80000000u : 0u);
    return h;
}

template <int CW>
__device__ __forceinline__ void qp_dequant(const QpCodes<CW>& c, const QpHead& h,
                                           float (&d)[QP_RUN]) {
    if (h.mag >> 31) {
        const uint32_t mag = h.mag & 0x7FFFFFFFu;
#pragma unroll
        for (int u = 0; u < QP_RUN; ++u) d[u] = __uint_as_float(mag | (qp_code<CW>(c, u) << 31));
    } else {
#pragma unroll
        for (int u = 0; u < QP_RUN; ++u) d[u] = ((float)qp_code<CW>(c, u) - h.fzp) * h.fs;
    }
}

__device__ __forceinline__ bool qp_aligned16(const void* p) {
    return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

// A run of fp32 row values: four 16-byte accesses when the run is whole and p allows them.
__device__ __forceinline__ void qp_load_f32(const float* p, int n, float fill,
                                            float (&v)[QP_RUN]) {
    if (n == QP_RUN && qp_aligned16(p)) {
#pragma unroll
        for (int q = 0; q < QP_RUN / 4; ++q) {
            const float4 t = reinterpret_cast<const float4*>(p)[q];
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int u = 0; u < QP_RUN; ++u) v[u] = u < n ? p[u] : fill;
    }
}

__device__ __forceinline__ void qp_store_f32(float* p, int n, const float (&v)[QP_RUN]) {
    if (n == QP_RUN && qp_aligned16(p)) {
#pragma unroll
        for (int q = 0; q < QP_RUN / 4; ++q)
            reinterpret_cast<float4*>(p)[q] =
                make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    } else {
#pragma unroll
        for (int u = 0; u < QP_RUN; ++u)
            if (u < n) p[u] = v[u];
    }
}

// ------------------------------------------------------------------ pack
template <int CW>
__global__ void __launch_bounds__(QP_THREADS)
quant_pack_kernel(const uint8_t* __restrict__ codes, int64_t c_cs, const int64_t* __restrict__ zp,
                  const float* __restrict__ x, int64_t x_cs, const float* __restrict__ base,
                  int64_t b_cs, uint8_t* __restrict__ packed, int64_t p_cs,
                  float* __restrict__ passv, const int64_t* __restrict__ seg_offsets,
                  const int32_t* __restrict__ chunk_offsets, const int64_t* __restrict__ boff,
                  int nseg) {
    const int z = blockIdx.y;
    const QpSub g = qp_sub(seg_offsets, chunk_offsets, nseg, blockIdx.x);
    if (g.len == 0) return;
    const int flag = zp[(int64_t)z * nseg + g.s] == INT64_MIN;
    const float* xr = x + z * x_cs;
    const float* br = base ? base + z * b_cs : nullptr;
    if (g.c0 == 0 && threadIdx.x == 0) {  // one writer per (client, segment)
        const float v0 = br ? xr[g.e0] - br[g.e0] : xr[g.e0];
        passv[(int64_t)z * nseg + g.s] = flag ? v0 : 0.f;
    }
    const int t0 = (int)threadIdx.x * QP_RUN;
    const int n = min(QP_RUN, g.len - t0);
    if (n <= 0) return;
    const int64_t e = g.e0 + t0;
    QpCodes<CW> c;
#pragma unroll
    for (int q = 0; q < QpCodes<CW>::NW; ++q) c.w[q] = 0u;
    if (flag) {  // the sign bits of the v the quantiser passed through
#pragma unroll
        for (int u = 0; u < QP_RUN; ++u)
            if (u < n) {
                const float v = br ? xr[e + u] - br[e + u] : xr[e + u];
                c.w[(u * CW) >> 5] |= (__float_as_uint(v) >> 31) << ((u * CW) & 31);
            }
    } else {
        const uint8_t* cr = codes + z * c_cs + e;
        uint32_t b4[QP_RUN / 4];
        if (n == QP_RUN && qp_aligned16(cr)) {
            const uint4 v = *reinterpret_cast<const uint4*>(cr);
            b4[0] = v.x; b4[1] = v.y; b4[2] = v.z; b4[3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < QP_RUN / 4; ++q) b4[q] = 0u;
#pragma unroll
            for (int u = 0; u < QP_RUN; ++u)
                if (u < n) b4[u >> 2] |= (uint32_t)cr[u] << (8 * (u & 3));
        }
#pragma unroll
        for (int u = 0; u < QP_RUN; ++u) {
            const uint32_t code = (b4[u >> 2] >> (8 * (u & 3))) & ((1u << CW) - 1u);
            c.w[(u * CW) >> 5] |= code << ((u * CW) & 31);
        }
    }
    qp_store<CW>(packed + z * p_cs + boff[g.s] + (g.c0 + t0) * CW / 8, c, n);
}

// ------------------------------------------------------------------ validate
__global__ void __launch_bounds__(QP_THREADS)
quant_validate_kernel(const uint8_t* __restrict__ packed, int64_t p_cs,
                      const double* __restrict__ scale, const int64_t* __restrict__ zp,
                      const float* __restrict__ passv, const int64_t* __restrict__ seg_lens,
                      const int64_t* __restrict__ boff, int nseg, int cw, int bits,
                      int32_t* __restrict__ bad_out) {
    const int s = blockIdx.x, z = blockIdx.y;
    const int64_t at = (int64_t)z * nseg + s;
    int bad = 0;
    if (threadIdx.x == 0) {
        const double sc = scale[at];
        bad = !(sc >= 0.0) || !isfinite(sc);
        if (zp[at] == INT64_MIN && !isfinite(passv[at])) bad = 1;
    }
    // the code bits at or above 2^bits, per byte; none where bits == cw
    const uint32_t cmask = (1u << cw) - 1u;
    const uint32_t hi = (cmask << bits) & cmask;
    const uint32_t m8 = cw == 8 ? hi : (cw == 4 ? (hi | hi << 4) : 0u);
    if (m8) {
        const uint8_t* pr = packed + z * p_cs + boff[s];
        const int64_t nbits = seg_lens[s] * cw;
        const int64_t whole = nbits >> 3;  // bytes every bit of which is a code
        const int64_t nv = whole >> 4;
        const uint32_t m32 = m8 * 0x01010101u;
        for (int64_t q = threadIdx.x; q < nv; q += QP_THREADS) {
            const uint4 v = reinterpret_cast<const uint4*>(pr)[q];
            if ((v.x | v.y | v.z | v.w) & m32) bad = 1;
        }
        for (int64_t b = (nv << 4) + threadIdx.x; b < whole; b += QP_THREADS)
            if (pr[b] & m8) bad = 1;
        const int used = (int)(nbits & 7);  // the last byte's code bits; the rest is padding
        if (used && threadIdx.x == 0 && (pr[whole] & m8 & ((1u << used) - 1u))) bad = 1;
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) bad_out[at] = bad ? 1 : 0;
}

// ------------------------------------------------------------------ unpack
// out and base carry no __restrict__: out may be the base rows (a lane reads its run of the base
// before it writes the same run of out).
template <int CW>
__global__ void __launch_bounds__(QP_THREADS)
quant_unpack_kernel(const uint8_t* __restrict__ packed, int64_t p_cs,
                    const double* __restrict__ scale, const int64_t* __restrict__ zp,
                    const float* __restrict__ passv, const float* base, int64_t b_cs, float* out,
                    int64_t o_cs, const int64_t* __restrict__ seg_offsets,
                    const int32_t* __restrict__ chunk_offsets, const int64_t* __restrict__ boff,
                    int nseg) {
    const int z = blockIdx.y;
    const QpSub g = qp_sub(seg_offsets, chunk_offsets, nseg, blockIdx.x);
    const int t0 = (int)threadIdx.x * QP_RUN;
    const int n = min(QP_RUN, g.len - t0);
    if (n <= 0) return;
    const QpHead h = qp_head(scale, zp, passv, (int64_t)z * nseg + g.s);
    const QpCodes<CW> c = qp_load<CW>(packed + z * p_cs + boff[g.s] + (g.c0 + t0) * CW / 8, n);
    float d[QP_RUN], b[QP_RUN];
    qp_dequant<CW>(c, h, d);
    const int64_t e = g.e0 + t0;
    if (base) {
        qp_load_f32(base + z * b_cs + e, n, 0.f, b);
#pragma unroll
        for (int u = 0; u < QP_RUN; ++u) d[u] = b[u] + d[u];
    }
    qp_store_f32(out + z * o_cs + e, n, d);
}

// ------------------------------------------------------------------ FedAvg from the codes
template <int CW>
struct QpSlot {
    QpCodes<CW> c;
    QpHead h;
    float w;
};

template <int CW>
__global__ void __launch_bounds__(QP_THREADS)
quant_fedavg_kernel(const uint8_t* __restrict__ packed, int64_t p_cs,
                    const double* __restrict__ scale, const int64_t* __restrict__ zp,
                    const float* __restrict__ passv, const int32_t* __restrict__ row_index,
                    const float* __restrict__ weights, int C, const float* __restrict__ base,
                    const int64_t* __restrict__ seg_offsets,
                    const int32_t* __restrict__ chunk_offsets, const int64_t* __restrict__ boff,
                    int nseg, float* __restrict__ out, int accumulate) {
    const QpSub g = qp_sub(seg_offsets, chunk_offsets, nseg, blockIdx.x);
    const int t0 = (int)threadIdx.x * QP_RUN;
    const int n = min(QP_RUN, g.len - t0);
    if (n <= 0) return;
    const int64_t e = g.e0 + t0;
    float acc[QP_RUN], b[QP_RUN];
    // without a base the dense row's element is d itself: -0.0 + d == d for every d
    if (base) {
        qp_load_f32(base + e, n, 0.f, b);
    } else {
#pragma unroll
        for (int u = 0; u < QP_RUN; ++u) b[u] = -0.f;
    }
    if (accumulate) {
        qp_load_f32(out + e, n, 0.f, acc);
    } else {
#pragma unroll
        for (int u = 0; u < QP_RUN; ++u) acc[u] = 0.f;
    }
    const uint8_t* p0 = packed + boff[g.s] + (g.c0 + t0) * CW / 8;
    auto fetch = [&](int k) {
        QpSlot<CW> sl;
        const int64_t r = row_index ? row_index[k] : k;
        sl.c = qp_load<CW>(p0 + r * p_cs, n);
        sl.h = qp_head(scale, zp, passv, r * nseg + g.s);
        sl.w = weights[k];
        return sl;
    };
    QpSlot<CW> ring[QP_PF];
#pragma unroll
    for (int u = 0; u < QP_PF; ++u)
        if (u < C) ring[u] = fetch(u);
    for (int k0 = 0; k0 < C; k0 += QP_PF) {
#pragma unroll
        for (int u = 0; u < QP_PF; ++u) {
            if (k0 + u < C) {
                const QpSlot<CW> sl = ring[u];
                if (k0 + u + QP_PF < C) ring[u] = fetch(k0 + u + QP_PF);
                float d[QP_RUN];
                qp_dequant<CW>(sl.c, sl.h, d);
#pragma unroll
                for (int q = 0; q < QP_RUN; ++q) {
                    const float xk = b[q] + d[q];     // the dense row's element
                    acc[q] = acc[q] + sl.w * xk;      // rounded multiply, rounded add
                }
            }
        }
    }
    qp_store_f32(out + e, n, acc);
}

static int qp_code_width(int bits) { return bits <= 1 ? 1 : bits == 2 ? 2 : bits <= 4 ? 4 : 8; }

static int qp_check_plan(const char* who, int32_t nclients, const int64_t* seg_offsets,
                         const int32_t* chunk_offsets, const int64_t* boff, int32_t nseg,
                         int32_t nchunks, int32_t bits) {
    FH_REQUIRE(nclients >= 0 && nseg > 0 && nchunks >= nseg, "%s: bad shape", who);
    FH_REQUIRE(bits >= 1 && bits <= 8, "%s: uint8 codes need bits in [1, 8] (got %d)", who, bits);
    FH_REQUIRE(nclients == 0 || (seg_offsets && chunk_offsets && boff), "%s: null pointer", who);
    FH_REQUIRE(fh_compress_chunk_elems() == QP_CHUNK, "%s: chunk size mismatch", who);
    FH_REQUIRE((int64_t)nchunks * QP_SUBS <= 0x7FFFFFFFll, "%s: too many chunks", who);
    return FH_OK;
}

// Aligned 16-byte loads are the point of the layout: a code row starts on a 16-byte boundary and
// so does the next one.
static int qp_check_rows(const char* who, const void* packed, int64_t packed_cs) {
    FH_REQUIRE(packed, "%s: null pointer", who);
    FH_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 15u) == 0 && packed_cs % 16 == 0,
               "%s: code rows must be 16-byte aligned with a stride that is a multiple of 16",
               who);
    return FH_OK;
}

#define QP_DISPATCH(kernel, cw, grid, st, ...)                                                  \
    do {                                                                                        \
        switch (cw) {                                                                           \
            case 1: FH_LAUNCH(kernel<1>, grid, dim3(QP_THREADS), 0, st, __VA_ARGS__); break;    \
            case 2: FH_LAUNCH(kernel<2>, grid, dim3(QP_THREADS), 0, st, __VA_ARGS__); break;    \
            case 4: FH_LAUNCH(kernel<4>, grid, dim3(QP_THREADS), 0, st, __VA_ARGS__); break;    \
            default: FH_LAUNCH(kernel<8>, grid, dim3(QP_THREADS), 0, st, __VA_ARGS__); break;   \
        }                                                                                       \
    } while (0)

}  // namespace fh

using namespace fh;

extern "C" int fh_quant_pack_rows(const uint8_t* codes, int64_t codes_cs, const int64_t* zp,
                                  const float* x, int64_t x_cs, const float* base,
                                  int64_t base_cs, uint8_t* packed, int64_t packed_cs,
                                  float* passv, int32_t nclients, const int64_t* seg_offsets,
                                  const int32_t* chunk_offsets, const int64_t* boff, int32_t nseg,
                                  int32_t nchunks, int32_t bits, void* stream) {
    if (int rc = qp_check_plan("quant_pack_rows", nclients, seg_offsets, chunk_offsets, boff, nseg,
                               nchunks, bits))
        return rc;
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(codes && zp && x && passv, "quant_pack_rows: null pointer");
    if (int rc = qp_check_rows("quant_pack_rows", packed, packed_cs)) return rc;
    const dim3 grid(nchunks * QP_SUBS, nclients);
    QP_DISPATCH(quant_pack_kernel, qp_code_width(bits), grid, as_stream(stream), codes, codes_cs,
                zp, x, x_cs, base, base_cs, packed, packed_cs, passv, seg_offsets, chunk_offsets,
                boff, nseg);
    FH_LAUNCH_CHECK("quant_pack_rows");
    return FH_OK;
}

extern "C" int fh_quant_validate(const uint8_t* packed, int64_t packed_cs, const double* scale,
                                 const int64_t* zp, const float* passv, int32_t nclients,
                                 const int64_t* seg_lens, const int64_t* boff, int32_t nseg,
                                 int32_t bits, int32_t* bad_out, void* stream) {
    FH_REQUIRE(nclients >= 0 && nseg > 0, "quant_validate: bad shape");
    FH_REQUIRE(bits >= 1 && bits <= 8, "quant_validate: uint8 codes need bits in [1, 8] (got %d)",
               bits);
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(scale && zp && passv && seg_lens && boff && bad_out, "quant_validate: null pointer");
    if (int rc = qp_check_rows("quant_validate", packed, packed_cs)) return rc;
    FH_LAUNCH(quant_validate_kernel, dim3(nseg, nclients), dim3(QP_THREADS), 0, as_stream(stream),
              packed, packed_cs, scale, zp, passv, seg_lens, boff, nseg, qp_code_width(bits), bits,
              bad_out);
    FH_LAUNCH_CHECK("quant_validate");
    return FH_OK;
}

extern "C" int fh_quant_unpack_rows(const uint8_t* packed, int64_t packed_cs, const double* scale,
                                    const int64_t* zp, const float* passv, const float* base,
                                    int64_t base_cs, float* out, int64_t out_cs, int32_t nclients,
                                    const int64_t* seg_offsets, const int32_t* chunk_offsets,
                                    const int64_t* boff, int32_t nseg, int32_t nchunks,
                                    int32_t bits, void* stream) {
    if (int rc = qp_check_plan("quant_unpack_rows", nclients, seg_offsets, chunk_offsets, boff,
                               nseg, nchunks, bits))
        return rc;
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(scale && zp && passv && out, "quant_unpack_rows: null pointer");
    if (int rc = qp_check_rows("quant_unpack_rows", packed, packed_cs)) return rc;
    FH_REQUIRE(out != base || base_cs != 0,
               "quant_unpack_rows: out may not alias a broadcast base row");
    const dim3 grid(nchunks * QP_SUBS, nclients);
    QP_DISPATCH(quant_unpack_kernel, qp_code_width(bits), grid, as_stream(stream), packed,
                packed_cs, scale, zp, passv, base, base_cs, out, out_cs, seg_offsets,
                chunk_offsets, boff, nseg);
    FH_LAUNCH_CHECK("quant_unpack_rows");
    return FH_OK;
}

extern "C" int fh_quant_fedavg(const uint8_t* packed, int64_t packed_cs, const double* scale,
                               const int64_t* zp, const float* passv, const int32_t* row_index,
                               const float* weights, int32_t num_clients, const float* base,
                               const int64_t* seg_offsets, const int32_t* chunk_offsets,
                               const int64_t* boff, int32_t nseg, int32_t nchunks, int32_t bits,
                               float* out, int32_t accumulate, void* stream) {
    if (int rc = qp_check_plan("quant_fedavg", 1, seg_offsets, chunk_offsets, boff, nseg, nchunks,
                               bits))
        return rc;
    FH_REQUIRE(num_clients >= 0, "quant_fedavg: bad client count %d", num_clients);
    FH_REQUIRE(out && (num_clients == 0 || (scale && zp && passv && weights)),
               "quant_fedavg: null pointer");
    if (num_clients > 0)
        if (int rc = qp_check_rows("quant_fedavg", packed, packed_cs)) return rc;
    FH_REQUIRE(out != base, "quant_fedavg: out may not alias base");
    const dim3 grid(nchunks * QP_SUBS);
    QP_DISPATCH(quant_fedavg_kernel, qp_code_width(bits), grid, as_stream(stream), packed,
                packed_cs, scale, zp, passv, row_index, weights, num_clients, base, seg_offsets,
                chunk_offsets, boff, nseg, out, accumulate);
    FH_LAUNCH_CHECK("quant_fedavg");
    return FH_OK;
}
