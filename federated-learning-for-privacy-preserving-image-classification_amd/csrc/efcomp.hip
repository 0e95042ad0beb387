// efcomp.hip — error feedback and stochastic rounding for the update compressors of
// compress.hip.  Not in the reference; the definition lives in include/fedhip.h.
//
// Error feedback (Stich et al. 2018; Karimireddy et al. 2019): every client keeps the part of its
// update that compression removed (the residual row) and adds it to its next update.
//   fh_ef_fold          resid <- fl32(fl32(x - base) + resid)            = v, the compensated update
//   fh_ef_topk_finish   after fh_topk_rows(v) wrote the keep mask: x_out = base + (keep ? v : 0),
//                       resid <- keep ? +0 : v
//   fh_ef_quant_finish  after fh_quantize_rows(v) wrote c: x_out = base + c, resid <- v - c
// Stochastic rounding (QSGD, Alistarh et al. 2017):
//   fh_squant_rows      per-chunk min/max, then q = floor(v / scale) + [Philox word < fraction]
//
// Work decomposition as compress.hip's: a (chunk, client) grid, every workgroup owns one
// CHUNK-element piece of one segment and finds the segment by binary search in chunk_offsets.
// Everything is HBM-bound element work.  A workgroup takes the 16-byte path when every tensor of
// the launch sits at the same offset from a 16-byte boundary at the chunk's first element (and
// the byte tensors at a 4-byte boundary one head further): scalar head up to the boundary,
// float4 / uchar4 body, scalar tail; otherwise one element per thread throughout.  The two paths
// run the same per-element functions, so they give the same bits.  The TU is built with
// -ffp-contract=off and has no fmaf: every fp32 operation is rounded on its own.
#include "fh_common.h"

namespace fh {

static constexpr int EF_CHUNK = 8192;  // == fh_compress_chunk_elems() (checked at launch)
static constexpr int EF_THREADS = 256;

__device__ __forceinline__ int ef_seg_of_chunk(const int32_t* __restrict__ chunk_offsets, int nseg,
                                               int chunk) {
    int lo = 0, hi = nseg - 1;  // largest s with chunk_offsets[s] <= chunk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (chunk_offsets[mid] <= chunk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The chunk's element range [e0, e1) inside segment s of a row.
struct EfRange {
    int s;
    int64_t e0, e1;
};

__device__ __forceinline__ EfRange ef_range(const int64_t* __restrict__ seg_offsets,
                                            const int32_t* __restrict__ chunk_offsets, int nseg,
                                            int chunk) {
    EfRange r;
    r.s = ef_seg_of_chunk(chunk_offsets, nseg, chunk);
    const int64_t s0 = seg_offsets[r.s], s1 = seg_offsets[r.s + 1];
    r.e0 = s0 + (int64_t)(chunk - chunk_offsets[r.s]) * EF_CHUNK;
    r.e1 = min(r.e0 + (int64_t)EF_CHUNK, s1);
    return r;
}

// Alignment of a launch's row pointers at one element: every non-null fp32 pointer must share
// the offset `mis` (in floats) from a 16-byte boundary, every non-null byte pointer must be
// 4-byte aligned `head` elements later.
struct EfAlign {
    unsigned mis = 0;
    bool any = false, ok = true;
    __device__ __forceinline__ void f32(const void* p) {
        if (!p) return;
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        const unsigned m = (unsigned)(a >> 2) & 3u;
        if ((a & 3u) != 0 || (any && m != mis)) ok = false;
        mis = m;
        any = true;
    }
    __device__ __forceinline__ int64_t head() const { return (int64_t)((4u - mis) & 3u); }
    __device__ __forceinline__ void u8(const void* p) {  // after every f32()
        if (!p) return;
        if (((reinterpret_cast<uintptr_t>(p) + (uintptr_t)head()) & 3u) != 0) ok = false;
    }
};

// One chunk: scalar(i) for single elements, vec4(i) for four consecutive ones that start on the
// common 16-byte boundary.
template <typename S, typename V>
__device__ __forceinline__ void ef_chunk_pass(int64_t e0, int64_t e1, bool vec, int64_t head,
                                              S scalar, V vec4) {
    const int tid = threadIdx.x;
    if (!vec) {
        for (int64_t i = e0 + tid; i < e1; i += EF_THREADS) scalar(i);
        return;
    }
    const int64_t h = min(head, e1 - e0);
    const int64_t b0 = e0 + h, nb = (e1 - b0) >> 2;
    for (int64_t q = tid; q < nb; q += EF_THREADS) vec4(b0 + 4 * q);
    if (tid < h) scalar(e0 + tid);
    const int64_t t = b0 + 4 * nb + tid;  // at most 3 left
    if (t < e1) scalar(t);
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ uchar4 ld4b(const uint8_t* p) { return *reinterpret_cast<const uchar4*>(p); }
__device__ __forceinline__ void st4b(uint8_t* p, const uchar4& v) { *reinterpret_cast<uchar4*>(p) = v; }

// ------------------------------------------------------------------ fold
__device__ __forceinline__ float ef_fold1(float x, float b, bool sub, float r) {
    const float d = sub ? (x - b) : x;
    return d + r;
}

__global__ void __launch_bounds__(EF_THREADS)
ef_fold_kernel(const float* __restrict__ x, int64_t x_cs, const float* __restrict__ base,
               int64_t b_cs, float* __restrict__ resid, int64_t r_cs,
               const int64_t* __restrict__ seg_offsets, const int32_t* __restrict__ chunk_offsets,
               int nseg) {
    const int z = blockIdx.y;
    const EfRange rg = ef_range(seg_offsets, chunk_offsets, nseg, blockIdx.x);
    const float* xr = x + z * x_cs;
    const float* br = base ? base + z * b_cs : nullptr;
    float* rr = resid + z * r_cs;
    const bool sub = br != nullptr;
    EfAlign al;
    al.f32(xr + rg.e0);
    al.f32(br ? br + rg.e0 : nullptr);
    al.f32(rr + rg.e0);
    ef_chunk_pass(
        rg.e0, rg.e1, al.ok, al.head(),
        [&](int64_t i) { rr[i] = ef_fold1(xr[i], sub ? br[i] : 0.f, sub, rr[i]); },
        [&](int64_t i) {
            const float4 a = ld4(xr + i), r = ld4(rr + i);
            float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
            if (sub) b = ld4(br + i);
            st4(rr + i, make_float4(ef_fold1(a.x, b.x, sub, r.x), ef_fold1(a.y, b.y, sub, r.y),
                                    ef_fold1(a.z, b.z, sub, r.z), ef_fold1(a.w, b.w, sub, r.w)));
        });
}

// ------------------------------------------------------------------ top-k finish
// d = keep ? v : +0; x_out = base + d (d without a base), as topk_apply_kernel; resid = keep ? +0 : v
__device__ __forceinline__ void ef_topk1(float v, uint8_t k, float b, bool add, float& xo,
                                         float& ro) {
    const float d = k ? v : 0.f;
    xo = add ? (b + d) : d;
    ro = k ? 0.f : v;
}

// x_out and base carry no __restrict__: x_out may be the base rows.
__global__ void __launch_bounds__(EF_THREADS)
ef_topk_finish_kernel(const float* base, int64_t b_cs, const uint8_t* __restrict__ keep,
                      int64_t k_cs, float* __restrict__ resid, int64_t r_cs, float* x_out,
                      int64_t o_cs, const int64_t* __restrict__ seg_offsets,
                      const int32_t* __restrict__ chunk_offsets, int nseg) {
    const int z = blockIdx.y;
    const EfRange rg = ef_range(seg_offsets, chunk_offsets, nseg, blockIdx.x);
    const float* br = base ? base + z * b_cs : nullptr;
    const uint8_t* kr = keep + z * k_cs;
    float* rr = resid + z * r_cs;
    float* orow = x_out + z * o_cs;
    const bool add = br != nullptr;
    EfAlign al;
    al.f32(br ? br + rg.e0 : nullptr);
    al.f32(rr + rg.e0);
    al.f32(orow + rg.e0);
    al.u8(kr + rg.e0);
    ef_chunk_pass(
        rg.e0, rg.e1, al.ok, al.head(),
        [&](int64_t i) {
            float xo, ro;
            ef_topk1(rr[i], kr[i], add ? br[i] : 0.f, add, xo, ro);
            orow[i] = xo;
            rr[i] = ro;
        },
        [&](int64_t i) {
            const float4 v = ld4(rr + i);
            const uchar4 k = ld4b(kr + i);
            float4 b = make_float4(0.f, 0.f, 0.f, 0.f), xo, ro;
            if (add) b = ld4(br + i);
            ef_topk1(v.x, k.x, b.x, add, xo.x, ro.x);
            ef_topk1(v.y, k.y, b.y, add, xo.y, ro.y);
            ef_topk1(v.z, k.z, b.z, add, xo.z, ro.z);
            ef_topk1(v.w, k.w, b.w, add, xo.w, ro.w);
            st4(orow + i, xo);
            st4(rr + i, ro);
        });
}

// ------------------------------------------------------------------ quantiser finish
// c, x_out and base carry no __restrict__: x_out may be c (every element is read before it is
// written, by the thread that writes it).
__global__ void __launch_bounds__(EF_THREADS)
ef_quant_finish_kernel(const float* base, int64_t b_cs, const float* c, int64_t c_cs,
                       float* __restrict__ resid, int64_t r_cs, float* x_out, int64_t o_cs,
                       const int64_t* __restrict__ seg_offsets,
                       const int32_t* __restrict__ chunk_offsets, int nseg) {
    const int z = blockIdx.y;
    const EfRange rg = ef_range(seg_offsets, chunk_offsets, nseg, blockIdx.x);
    const float* br = base ? base + z * b_cs : nullptr;
    const float* cr = c + z * c_cs;
    float* rr = resid + z * r_cs;
    float* orow = x_out + z * o_cs;
    const bool add = br != nullptr;
    EfAlign al;
    al.f32(br ? br + rg.e0 : nullptr);
    al.f32(cr + rg.e0);
    al.f32(rr + rg.e0);
    al.f32(orow + rg.e0);
    ef_chunk_pass(
        rg.e0, rg.e1, al.ok, al.head(),
        [&](int64_t i) {
            const float q = cr[i], v = rr[i];
            orow[i] = add ? (br[i] + q) : q;
            rr[i] = v - q;
        },
        [&](int64_t i) {
            const float4 q = ld4(cr + i), v = ld4(rr + i);
            float4 xo = q;
            if (add) {
                const float4 b = ld4(br + i);
                xo = make_float4(b.x + q.x, b.y + q.y, b.z + q.z, b.w + q.w);
            }
            st4(orow + i, xo);
            st4(rr + i, make_float4(v.x - q.x, v.y - q.y, v.z - q.z, v.w - q.w));
        });
}

// ------------------------------------------------------------------ stochastic quantiser
// v of one element: the folded residual when given (x is not read), else x - base.
__device__ __forceinline__ float sq_v1(float x, float b, bool sub) { return sub ? (x - b) : x; }

__global__ void __launch_bounds__(EF_THREADS)
squant_minmax_kernel(const float* __restrict__ x, int64_t x_cs, const float* __restrict__ base,
                     int64_t b_cs, const int64_t* __restrict__ seg_offsets,
                     const int32_t* __restrict__ chunk_offsets, int nseg, int nchunks,
                     float2* __restrict__ partial) {
    const int chunk = blockIdx.x, z = blockIdx.y;
    const EfRange rg = ef_range(seg_offsets, chunk_offsets, nseg, chunk);
    const float* xr = x + z * x_cs;
    const float* br = base ? base + z * b_cs : nullptr;
    const bool sub = br != nullptr;
    EfAlign al;
    al.f32(xr + rg.e0);
    al.f32(br ? br + rg.e0 : nullptr);
    float mn = INFINITY, mx = -INFINITY;
    ef_chunk_pass(
        rg.e0, rg.e1, al.ok, al.head(),
        [&](int64_t i) {
            const float v = sq_v1(xr[i], sub ? br[i] : 0.f, sub);
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        },
        [&](int64_t i) {
            const float4 a = ld4(xr + i);
            float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
            if (sub) b = ld4(br + i);
            const float v0 = sq_v1(a.x, b.x, sub), v1 = sq_v1(a.y, b.y, sub),
                        v2 = sq_v1(a.z, b.z, sub), v3 = sq_v1(a.w, b.w, sub);
            mn = fminf(fminf(mn, fminf(v0, v1)), fminf(v2, v3));
            mx = fmaxf(fmaxf(mx, fmaxf(v0, v1)), fmaxf(v2, v3));
        });
    __shared__ float smn[EF_THREADS / 64], smx[EF_THREADS / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {  // min / max: any order, the same value
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { smn[wid] = mn; smx[wid] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[(int64_t)z * nchunks + chunk] =
            make_float2(fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3])),
                        fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3])));
    }
}

struct SqParams {
    float scale, lo, top, bot;  // q is clamped to [bot, top]; lo = 0 in symmetric mode
    int code_bias;              // codes = q + code_bias
    int asym;
};

// One element.  r: its 32-bit random word.
__device__ __forceinline__ void sq_elem(float v, uint32_t r, const SqParams& p, float& deq,
                                        uint8_t& code) {
    if (!(p.scale > 0.f)) {  // constant / all-zero / one-element segment: pass through
        deq = v;
        code = 0;
        return;
    }
    const float u = p.asym ? (v - p.lo) : v;
    const float t = __fdiv_rn(u, p.scale);
    const float fl = floorf(t);
    const float f = t - fl;                                // in [0, 1]
    const uint32_t thr = (uint32_t)(f * 16777216.0f);      // exact product, truncated
    const float up = ((r >> 8) < thr) ? 1.f : 0.f;
    const float q = fminf(fmaxf(fl + up, p.bot), p.top);   // integers below 2^17: exact
    const float d = q * p.scale;
    deq = p.asym ? (p.lo + d) : d;
    code = (uint8_t)((int)q + p.code_bias);
}

__device__ __forceinline__ uint32_t sq_word(const uint4& w, unsigned u) {
    return u == 0 ? w.x : (u == 1 ? w.y : (u == 2 ? w.z : w.w));
}

// x / out and resid / resid_out may alias: no __restrict__ on them.
__global__ void __launch_bounds__(EF_THREADS)
squant_apply_kernel(const float* x, int64_t x_cs, const float* base, int64_t b_cs, int v_is_x,
                    float* out, int64_t o_cs, uint8_t* __restrict__ codes, int64_t c_cs,
                    float* resid_out, int64_t ro_cs, const int64_t* __restrict__ seg_offsets,
                    const int32_t* __restrict__ chunk_offsets, int nseg, int nchunks,
                    const float2* __restrict__ partial, int bits, int symmetric, uint64_t key,
                    const int64_t* __restrict__ ids, const uint32_t* __restrict__ words,
                    int64_t w_cs, float* __restrict__ scale_out, float* __restrict__ lo_out) {
    const int chunk = blockIdx.x, z = blockIdx.y;
    const EfRange rg = ef_range(seg_offsets, chunk_offsets, nseg, chunk);
    const int s = rg.s;
    __shared__ float s_mn, s_mx;
    if (threadIdx.x < 64) {  // the segment's min / max from its chunks' partials
        float mn = INFINITY, mx = -INFINITY;
        for (int c = chunk_offsets[s] + (int)threadIdx.x; c < chunk_offsets[s + 1]; c += 64) {
            const float2 p = partial[(int64_t)z * nchunks + c];
            mn = fminf(mn, p.x);
            mx = fmaxf(mx, p.y);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, o, 64));
            mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        }
        if (threadIdx.x == 0) { s_mn = mn; s_mx = mx; }
    }
    __syncthreads();
    SqParams p;
    p.asym = !symmetric;
    if (symmetric) {
        const float qmax = (float)((1 << (bits - 1)) - 1);
        p.scale = __fdiv_rn(fmaxf(fabsf(s_mn), fabsf(s_mx)), qmax);
        p.lo = 0.f;
        p.top = qmax;
        p.bot = -qmax;
        p.code_bias = (int)qmax;
    } else {
        const float L = (float)((1 << bits) - 1);
        p.scale = __fdiv_rn(s_mx - s_mn, L);
        p.lo = s_mn;
        p.top = L;
        p.bot = 0.f;
        p.code_bias = 0;
    }
    if (threadIdx.x == 0 && chunk == chunk_offsets[s]) {  // one writer per (client, segment)
        if (scale_out) scale_out[(int64_t)z * nseg + s] = p.scale;
        if (lo_out) lo_out[(int64_t)z * nseg + s] = p.lo;
    }
    // v_is_x: v = x - base.  Otherwise x holds the folded residual (v itself).
    const float* xr = x + z * x_cs;
    const float* br = base ? base + z * b_cs : nullptr;
    float* orow = out ? out + z * o_cs : nullptr;
    uint8_t* crow = codes ? codes + z * c_cs : nullptr;
    float* rrow = resid_out ? resid_out + z * ro_cs : nullptr;
    const uint32_t* wr = words ? words + z * w_cs : nullptr;
    const bool sub = v_is_x && br != nullptr, add = br != nullptr;
    const uint64_t hi = (uint64_t)ids[z] | FH_SQUANT_STREAM_BIT;
    EfAlign al;
    al.f32(xr + rg.e0);
    al.f32(br ? br + rg.e0 : nullptr);
    al.f32(orow ? orow + rg.e0 : nullptr);
    al.f32(rrow ? rrow + rg.e0 : nullptr);
    al.u8(crow ? crow + rg.e0 : nullptr);
    ef_chunk_pass(
        rg.e0, rg.e1, al.ok, al.head(),
        [&](int64_t i) {
            const float b = add ? br[i] : 0.f;
            const float v = sq_v1(xr[i], b, sub);
            const uint32_t r = wr ? wr[i]
                                  : sq_word(Philox::gen(key, hi, (uint64_t)i >> 2), (unsigned)i & 3u);
            float d;
            uint8_t cd;
            sq_elem(v, r, p, d, cd);
            if (crow) crow[i] = cd;
            if (orow) orow[i] = add ? (b + d) : d;
            if (rrow) rrow[i] = v - d;
        },
        [&](int64_t i) {
            const float4 a = ld4(xr + i);
            float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
            if (add) b = ld4(br + i);
            const float v[4] = {sq_v1(a.x, b.x, sub), sq_v1(a.y, b.y, sub), sq_v1(a.z, b.z, sub),
                                sq_v1(a.w, b.w, sub)};
            uint32_t r[4];
            if (wr) {
#pragma unroll
                for (int u = 0; u < 4; ++u) r[u] = wr[i + u];
            } else {
                // element j draws word j & 3 of counter j >> 2: one block when i is a multiple
                // of 4 (rows that start on a 16-byte boundary), else the block's tail and the
                // next block's head
                const unsigned o = (unsigned)i & 3u;
                const uint4 w0 = Philox::gen(key, hi, (uint64_t)i >> 2);
                if (o == 0) {
                    r[0] = w0.x; r[1] = w0.y; r[2] = w0.z; r[3] = w0.w;
                } else {
                    const uint4 w1 = Philox::gen(key, hi, ((uint64_t)i >> 2) + 1);
#pragma unroll
                    for (unsigned u = 0; u < 4; ++u)
                        r[u] = (o + u < 4) ? sq_word(w0, o + u) : sq_word(w1, o + u - 4);
                }
            }
            float d[4];
            uint8_t cd[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) sq_elem(v[u], r[u], p, d[u], cd[u]);
            if (crow) st4b(crow + i, make_uchar4(cd[0], cd[1], cd[2], cd[3]));
            if (orow)
                st4(orow + i, add ? make_float4(b.x + d[0], b.y + d[1], b.z + d[2], b.w + d[3])
                                  : make_float4(d[0], d[1], d[2], d[3]));
            if (rrow)
                st4(rrow + i, make_float4(v[0] - d[0], v[1] - d[1], v[2] - d[2], v[3] - d[3]));
        });
}

static int ef_check_plan(const char* who, int32_t nclients, const int64_t* seg_offsets,
                         const int32_t* chunk_offsets, int32_t nseg, int32_t nchunks) {
    FH_REQUIRE(nclients >= 0 && nseg > 0 && nchunks >= nseg, "%s: bad shape", who);
    FH_REQUIRE(nclients == 0 || (seg_offsets && chunk_offsets), "%s: null pointer", who);
    FH_REQUIRE(fh_compress_chunk_elems() == EF_CHUNK, "%s: chunk size mismatch", who);
    return FH_OK;
}

}  // namespace fh

using namespace fh;

extern "C" int fh_ef_fold(const float* x, int64_t x_cs, const float* base, int64_t base_cs,
                          float* resid, int64_t resid_cs, int32_t nclients,
                          const int64_t* seg_offsets, const int32_t* chunk_offsets, int32_t nseg,
                          int32_t nchunks, void* stream) {
    if (int rc = ef_check_plan("ef_fold", nclients, seg_offsets, chunk_offsets, nseg, nchunks))
        return rc;
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(x && resid, "ef_fold: null pointer");
    FH_LAUNCH(ef_fold_kernel, dim3(nchunks, nclients), dim3(EF_THREADS), 0, as_stream(stream), x,
              x_cs, base, base_cs, resid, resid_cs, seg_offsets, chunk_offsets, nseg);
    FH_LAUNCH_CHECK("ef_fold");
    return FH_OK;
}

extern "C" int fh_ef_topk_finish(const float* base, int64_t base_cs, const uint8_t* keep,
                                 int64_t keep_cs, float* resid, int64_t resid_cs, float* x_out,
                                 int64_t x_out_cs, int32_t nclients, const int64_t* seg_offsets,
                                 const int32_t* chunk_offsets, int32_t nseg, int32_t nchunks,
                                 void* stream) {
    if (int rc = ef_check_plan("ef_topk_finish", nclients, seg_offsets, chunk_offsets, nseg,
                               nchunks))
        return rc;
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(keep && resid && x_out, "ef_topk_finish: null pointer");
    FH_LAUNCH(ef_topk_finish_kernel, dim3(nchunks, nclients), dim3(EF_THREADS), 0,
              as_stream(stream), base, base_cs, keep, keep_cs, resid, resid_cs, x_out, x_out_cs,
              seg_offsets, chunk_offsets, nseg);
    FH_LAUNCH_CHECK("ef_topk_finish");
    return FH_OK;
}

extern "C" int fh_ef_quant_finish(const float* base, int64_t base_cs, const float* c, int64_t c_cs,
                                  float* resid, int64_t resid_cs, float* x_out, int64_t x_out_cs,
                                  int32_t nclients, const int64_t* seg_offsets,
                                  const int32_t* chunk_offsets, int32_t nseg, int32_t nchunks,
                                  void* stream) {
    if (int rc = ef_check_plan("ef_quant_finish", nclients, seg_offsets, chunk_offsets, nseg,
                               nchunks))
        return rc;
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(c && resid && x_out, "ef_quant_finish: null pointer");
    FH_REQUIRE(c != resid && resid != x_out, "ef_quant_finish: resid may not alias c or x_out");
    FH_LAUNCH(ef_quant_finish_kernel, dim3(nchunks, nclients), dim3(EF_THREADS), 0,
              as_stream(stream), base, base_cs, c, c_cs, resid, resid_cs, x_out, x_out_cs,
              seg_offsets, chunk_offsets, nseg);
    FH_LAUNCH_CHECK("ef_quant_finish");
    return FH_OK;
}

extern "C" int64_t fh_squant_workspace(int32_t nclients, int32_t nchunks) {
    return (int64_t)nclients * nchunks * (int64_t)sizeof(float2);
}

extern "C" int fh_squant_rows(const float* x, int64_t x_cs, const float* base, int64_t base_cs,
                              const float* resid, int64_t resid_cs, float* out, int64_t out_cs,
                              uint8_t* codes, int64_t codes_cs, float* resid_out,
                              int64_t resid_out_cs, int32_t nclients, const int64_t* seg_offsets,
                              const int32_t* chunk_offsets, int32_t nseg, int32_t nchunks,
                              int32_t bits, int32_t symmetric, uint64_t key, const int64_t* ids,
                              const uint32_t* words, int64_t words_cs, float* scale_out,
                              float* lo_out, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = ef_check_plan("squant_rows", nclients, seg_offsets, chunk_offsets, nseg, nchunks))
        return rc;
    FH_REQUIRE(bits >= 2 && bits <= 16, "squant_rows: bits must be in [2, 16] (got %d)", bits);
    FH_REQUIRE(!codes || bits <= 8, "squant_rows: uint8 codes need bits <= 8");
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(resid || x, "squant_rows: neither x nor resid");
    FH_REQUIRE(ids, "squant_rows: null client ids");
    FH_REQUIRE(ws && (int64_t)ws_bytes >= fh_squant_workspace(nclients, nchunks),
               "squant_rows: workspace too small");
    float2* partial = reinterpret_cast<float2*>(ws);
    hipStream_t st = as_stream(stream);
    dim3 grid(nchunks, nclients);
    // with a residual, v is the residual itself: the kernels read it through the x slot
    const float* vin = resid ? resid : x;
    const int64_t vin_cs = resid ? resid_cs : x_cs;
    const int v_is_x = resid ? 0 : 1;
    FH_LAUNCH(squant_minmax_kernel, grid, dim3(EF_THREADS), 0, st, vin, vin_cs,
              v_is_x ? base : (const float*)nullptr, base_cs, seg_offsets, chunk_offsets, nseg,
              nchunks, partial);
    FH_LAUNCH_CHECK("squant_rows/minmax");
    FH_LAUNCH(squant_apply_kernel, grid, dim3(EF_THREADS), 0, st, vin, vin_cs, base, base_cs,
              v_is_x, out, out_cs, codes, codes_cs, resid_out, resid_out_cs, seg_offsets,
              chunk_offsets, nseg, nchunks, partial, bits, symmetric, key, ids, words, words_cs,
              scale_out, lo_out);
    FH_LAUNCH_CHECK("squant_rows/apply");
    return FH_OK;
}
