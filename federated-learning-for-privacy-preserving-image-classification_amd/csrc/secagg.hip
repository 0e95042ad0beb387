// secagg.hip — secure aggregation arithmetic (Bonawitz et al., CCS 2017): client rows encoded
// in fixed point in the ring Z/2^32 and covered by pairwise pseudorandom masks that cancel in
// the sum, and the server's sum / unmask / decode.  The reference repository has no such
// rule; the definitions live in include/fedhip.h and DESIGN.md §5.
//
// Both kernels work on "mask terms" (key, sign): the mask word of a term for coordinate j is
// word j % 4 (.x .y .z .w) of Philox::gen(key, nonce, j / 4).  A thread owns one Philox
// counter, i.e. four consecutive coordinates, and walks the terms; the term list is the same
// for every lane of a workgroup, so keys and signs are scalar loads and the sign test is a
// uniform branch.  Integer multiplies dominate: per term and thread 10 rounds of two
// 32 x 32 -> 64 products.  Everything after the one fp32 multiply of the encoding is exact or
// an integer mod 2^32, so the results do not depend on the path (16-byte or scalar), the grid
// or the run.  The only atomic is the integer add of a workgroup's clip count.
#include "fh_common.h"

namespace fh {

constexpr int SA_MAX_TERMS = 64;     // per row in fh_secagg_encode_mask_rows
constexpr int64_t SA_MAX_GRID_Y = 65535;

// sum_t sign[t] * m(key[t], .) mod 2^32 for the four coordinates of Philox counter `ctr`
__device__ __forceinline__ uint4 sa_mask_sum(const uint64_t* __restrict__ keys,
                                             const int32_t* __restrict__ signs, int nterms,
                                             uint64_t nonce, uint64_t ctr) {
    uint4 s = make_uint4(0u, 0u, 0u, 0u);
    for (int t = 0; t < nterms; ++t) {
        const int32_t sg = signs[t];
        if (sg == 0) continue;
        const uint4 m = Philox::gen(keys[t], nonce, ctr);
        if (sg > 0) {
            s.x += m.x;
            s.y += m.y;
            s.z += m.z;
            s.w += m.w;
        } else {
            s.x -= m.x;
            s.y -= m.y;
            s.z -= m.z;
            s.w -= m.w;
        }
    }
    return s;
}

// fixed-point code of v: rint(v * 2^frac_bits) in fp64 (the product is exact), NaN -> 0,
// saturated to +-qmax; each of the three cases counts as clipped
__device__ __forceinline__ uint32_t sa_encode(float v, double scale, double qmax, int& bad) {
    double r = rint((double)v * scale);
    if (r != r) {
        r = 0.0;
        ++bad;
    } else if (r > qmax) {
        r = qmax;
        ++bad;
    } else if (r < -qmax) {
        r = -qmax;
        ++bad;
    }
    return (uint32_t)(int32_t)r;
}

// Thread u of a row: Philox counter q0 + u, coordinates 4 * (q0 + u) .. + 3 (those below P).
// VEC: every quad is whole and rows / out are 16-byte aligned (the host checks).
template <bool VEC>
__global__ void __launch_bounds__(256)
secagg_encode_kernel(const float* __restrict__ rows, int64_t row_stride,
                     const int32_t* __restrict__ row_index, const float* __restrict__ weights,
                     int num_rows, int64_t P, int64_t q0, int64_t nquads, double scale,
                     double qmax, const uint64_t* __restrict__ term_keys,
                     const int32_t* __restrict__ term_signs, int nterms, uint64_t nonce,
                     uint32_t* __restrict__ out, int64_t out_stride,
                     int32_t* __restrict__ clipped) {
    __shared__ int red[4];
    const int64_t u = blockIdx.x * (int64_t)256 + threadIdx.x;
    const int64_t q = q0 + u, j0 = q * 4;
    const int n = u < nquads ? (VEC ? 4 : (int)std::min<int64_t>(4, P - j0)) : 0;
    for (int z = blockIdx.y; z < num_rows; z += gridDim.y) {
        int bad = 0;
        if (n > 0) {
            const int64_t r = row_index ? row_index[z] : z;
            const float* xp = rows + r * row_stride + j0;
            uint32_t* op = out + (int64_t)z * out_stride + j0;
            float x[4] = {0.f, 0.f, 0.f, 0.f};
            if (VEC) {
                *reinterpret_cast<float4*>(x) = *reinterpret_cast<const float4*>(xp);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < n) x[i] = xp[i];
            }
            const uint4 m = sa_mask_sum(term_keys + (int64_t)z * nterms,
                                        term_signs + (int64_t)z * nterms, nterms, nonce,
                                        (uint64_t)q);
            uint32_t o[4] = {m.x, m.y, m.z, m.w};
            const bool hw = weights != nullptr;
            const float w = hw ? weights[z] : 1.f;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < n) o[i] += sa_encode(hw ? w * x[i] : x[i], scale, qmax, bad);  // no FMA
            if (VEC) {
                *reinterpret_cast<uint4*>(op) = *reinterpret_cast<const uint4*>(o);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < n) op[i] = o[i];
            }
        }
        if (clipped) {  // uniform: workgroup count, then one integer atomic (order-free)
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) bad += __shfl_xor(bad, s, 64);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bad;
            __syncthreads();
            if (threadIdx.x == 0) {
                const int tot = red[0] + red[1] + red[2] + red[3];
                if (tot) atomicAdd(clipped + z, tot);
            }
            __syncthreads();
        }
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256)
secagg_sum_decode_kernel(const uint32_t* __restrict__ masked, int64_t stride,
                         const int32_t* __restrict__ row_index, int num_rows, int64_t P,
                         int64_t q0, int64_t nquads, const uint64_t* __restrict__ term_keys,
                         const int32_t* __restrict__ term_signs, int nterms, uint64_t nonce,
                         double inv_scale, float* __restrict__ out,
                         uint32_t* __restrict__ sum_out) {
    const int64_t u = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (u >= nquads) return;
    const int64_t q = q0 + u, j0 = q * 4;
    const int n = VEC ? 4 : (int)std::min<int64_t>(4, P - j0);
    uint32_t a[4] = {0u, 0u, 0u, 0u};
    if (VEC) {
        int k = 0;
        for (; k + 4 <= num_rows; k += 4) {  // four rows in flight
            uint4 v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t r = row_index ? row_index[k + i] : (k + i);
                v[i] = *reinterpret_cast<const uint4*>(masked + r * stride + j0);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[0] += v[i].x;
                a[1] += v[i].y;
                a[2] += v[i].z;
                a[3] += v[i].w;
            }
        }
        for (; k < num_rows; ++k) {
            const int64_t r = row_index ? row_index[k] : k;
            const uint4 v = *reinterpret_cast<const uint4*>(masked + r * stride + j0);
            a[0] += v.x;
            a[1] += v.y;
            a[2] += v.z;
            a[3] += v.w;
        }
    } else {
        for (int k = 0; k < num_rows; ++k) {
            const int64_t r = row_index ? row_index[k] : k;
            const uint32_t* mp = masked + r * stride + j0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < n) a[i] += mp[i];
        }
    }
    const uint4 m = sa_mask_sum(term_keys, term_signs, nterms, nonce, (uint64_t)q);
    a[0] -= m.x;
    a[1] -= m.y;
    a[2] -= m.z;
    a[3] -= m.w;
    float f[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)  // int32 -> fp64 and the power-of-two scale are exact
        f[i] = (float)((double)(int32_t)a[i] * inv_scale);
    if (VEC) {
        if (sum_out) *reinterpret_cast<uint4*>(sum_out + j0) = *reinterpret_cast<const uint4*>(a);
        if (out) *reinterpret_cast<float4*>(out + j0) = *reinterpret_cast<const float4*>(f);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < n) {
                if (sum_out) sum_out[j0 + i] = a[i];
                if (out) out[j0 + i] = f[i];
            }
        }
    }
}

static inline bool sa_aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace fh

using namespace fh;

extern "C" int fh_secagg_encode_mask_rows(const float* rows, int64_t row_stride,
                                          const int32_t* row_index, const float* weights,
                                          int32_t num_rows, int64_t P, int32_t frac_bits,
                                          int32_t qmax, const uint64_t* term_keys,
                                          const int32_t* term_signs, int32_t nterms,
                                          uint64_t nonce, uint32_t* out, int64_t out_stride,
                                          int32_t* clipped, void* stream) {
    FH_REQUIRE(num_rows >= 1, "secagg_encode: num_rows=%d, need >= 1", num_rows);
    FH_REQUIRE(frac_bits >= 0 && frac_bits <= 30, "secagg_encode: frac_bits=%d outside [0, 30]",
               frac_bits);
    FH_REQUIRE(qmax >= 1, "secagg_encode: qmax=%d outside [1, 2^31 - 1]", qmax);
    FH_REQUIRE(nterms >= 0 && nterms <= SA_MAX_TERMS, "secagg_encode: nterms=%d outside [0, %d]",
               nterms, SA_MAX_TERMS);
    FH_REQUIRE(P >= 0 && row_stride >= 0 && out_stride >= 0,
               "secagg_encode: bad sizes P=%lld row_stride=%lld out_stride=%lld", (long long)P,
               (long long)row_stride, (long long)out_stride);
    if (P == 0) return FH_OK;
    FH_REQUIRE(rows && out && (nterms == 0 || (term_keys && term_signs)),
               "secagg_encode: null pointer");
    const int64_t nq = ceil_div(P, 4);
    FH_REQUIRE(ceil_div(nq, 256) <= 0x7FFFFFFF, "secagg_encode: P=%lld too large", (long long)P);
    hipStream_t st = as_stream(stream);
    const double scale = (double)(1u << frac_bits);
    const dim3 block(256);
    const unsigned gy = (unsigned)std::min<int64_t>(num_rows, SA_MAX_GRID_Y);
    const bool vec_ok = row_stride % 4 == 0 && out_stride % 4 == 0 && sa_aligned16(rows) &&
                        sa_aligned16(out);
    // 16-byte path over the whole quads, the scalar instance for the P % 4 tail (one quad)
    // or, when strides / bases rule the vector path out, for everything
    const int64_t vq = vec_ok ? P / 4 : 0;
    if (vq) {
        FH_LAUNCH(secagg_encode_kernel<true>, dim3((unsigned)ceil_div(vq, 256), gy), block, 0,
                  st, rows, row_stride, row_index, weights, num_rows, P, (int64_t)0, vq, scale,
                  (double)qmax, term_keys, term_signs, nterms, nonce, out, out_stride, clipped);
        FH_LAUNCH_CHECK("secagg_encode_vec");
    }
    if (vq < nq) {
        FH_LAUNCH(secagg_encode_kernel<false>, dim3((unsigned)ceil_div(nq - vq, 256), gy), block,
                  0, st, rows, row_stride, row_index, weights, num_rows, P, vq, nq - vq, scale,
                  (double)qmax, term_keys, term_signs, nterms, nonce, out, out_stride, clipped);
        FH_LAUNCH_CHECK("secagg_encode_scalar");
    }
    return FH_OK;
}

extern "C" int fh_secagg_sum_decode(const uint32_t* masked, int64_t stride,
                                    const int32_t* row_index, int32_t num_rows, int64_t P,
                                    const uint64_t* term_keys, const int32_t* term_signs,
                                    int32_t nterms, uint64_t nonce, int32_t frac_bits, float* out,
                                    uint32_t* sum_out, void* stream) {
    FH_REQUIRE(num_rows >= 1, "secagg_sum_decode: num_rows=%d, need >= 1", num_rows);
    FH_REQUIRE(frac_bits >= 0 && frac_bits <= 30,
               "secagg_sum_decode: frac_bits=%d outside [0, 30]", frac_bits);
    FH_REQUIRE(nterms >= 0, "secagg_sum_decode: nterms=%d, need >= 0", nterms);
    FH_REQUIRE(P >= 0 && stride >= 0, "secagg_sum_decode: bad sizes P=%lld stride=%lld",
               (long long)P, (long long)stride);
    if (P == 0) return FH_OK;
    FH_REQUIRE(out || sum_out, "secagg_sum_decode: one of out / sum_out must be given");
    FH_REQUIRE(masked && (nterms == 0 || (term_keys && term_signs)),
               "secagg_sum_decode: null pointer");
    const int64_t nq = ceil_div(P, 4);
    FH_REQUIRE(ceil_div(nq, 256) <= 0x7FFFFFFF, "secagg_sum_decode: P=%lld too large",
               (long long)P);
    hipStream_t st = as_stream(stream);
    const double inv_scale = 1.0 / (double)(1u << frac_bits);
    const dim3 block(256);
    const bool vec_ok = stride % 4 == 0 && sa_aligned16(masked) && sa_aligned16(out) &&
                        sa_aligned16(sum_out);  // NULL counts as aligned
    const int64_t vq = vec_ok ? P / 4 : 0;
    if (vq) {
        FH_LAUNCH(secagg_sum_decode_kernel<true>, dim3((unsigned)ceil_div(vq, 256)), block, 0, st,
                  masked, stride, row_index, num_rows, P, (int64_t)0, vq, term_keys, term_signs,
                  nterms, nonce, inv_scale, out, sum_out);
        FH_LAUNCH_CHECK("secagg_sum_decode_vec");
    }
    if (vq < nq) {
        FH_LAUNCH(secagg_sum_decode_kernel<false>, dim3((unsigned)ceil_div(nq - vq, 256)), block,
                  0, st, masked, stride, row_index, num_rows, P, vq, nq - vq, term_keys,
                  term_signs, nterms, nonce, inv_scale, out, sum_out);
        FH_LAUNCH_CHECK("secagg_sum_decode_scalar");
    }
    return FH_OK;
}
