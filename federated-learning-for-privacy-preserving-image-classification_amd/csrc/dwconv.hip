// dwconv.hip — depthwise 3x3 convolution (groups = channels, pad 1, stride 1 or 2, no bias):
// forward, input gradient and weight gradient of LightweightMobileNet's depthwise layers
// (reference models_pytorch.py: DepthwiseSeparableConv).
//
// There is no reduction over input channels, so these are HBM-bound VALU kernels: every
// activation element is read once from HBM and every result written once.  A thread owns
// four adjacent pixels of one row (one float4 of y / dX, or of dY in the weight gradient);
// its channel's nine weights live in registers (scalar loads: a weight is a view into a
// packed parameter row, only 4-byte aligned).
//
// Halo: the rows above and below are guarded loads (zero outside the map; the re-reads of a
// row by the threads of the neighbouring rows hit L1/L2, the lanes of one load instruction
// still cover contiguous 16-byte pieces); the columns left and right come from the
// neighbouring lanes' registers (wave shuffles) — a row of the map never straddles a wave
// (a row is at most 8 float4s, a wave starts on a multiple of 64), so no LDS, no barrier and
// no second pass over a staged tile are needed.  Every lane of a wave executes every shuffle:
// out-of-range lanes and images >= counts[client] are predicated (their loads are not
// issued, their stores skipped), never exited early.
//
// Determinism: no atomics.  The weight gradient is one workgroup per (client, channel,
// image split); the lanes' nine sums are combined by a wave butterfly and the four waves in
// order, and a split launch's partials are added in split order by a second small launch.
#include "fh_common.h"

namespace fh {

namespace {

struct DwGeom {
    int C, h, ho;        // channels, input map, output map (h / stride)
    int q4_shift;        // log2(float4s per tiled plane)
    int row_shift;       // log2(float4s per tiled-plane row)
    FastDiv divC;
};

__device__ __forceinline__ float4 ld4(const float* p, bool ok) {
    return ok ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// Stride 1: the 3 x 6 input window of output pixels (oy, ox0 .. ox0 + 3): col[r][0] is column
// ox0 - 1, col[r][5] column ox0 + 4.  Executed by every lane of the wave (shuffles).
__device__ __forceinline__ void window_s1(const float* __restrict__ plane, int h, int oy, int ox0,
                                          bool valid, float col[3][6]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int iy = oy - 1 + r;
        const bool ok = valid && iy >= 0 && iy < h;
        const float4 v = ld4(plane + iy * h + ox0, ok);
        const float l = __shfl_up(v.w, 1, 64), rt = __shfl_down(v.x, 1, 64);
        col[r][0] = ox0 > 0 ? l : 0.f;
        col[r][1] = v.x; col[r][2] = v.y; col[r][3] = v.z; col[r][4] = v.w;
        col[r][5] = ox0 + 4 < h ? rt : 0.f;
    }
}

// Stride 2: the 3 x 9 input window of output pixels (oy, ox0 .. ox0 + 3): col[r][0] is input
// column 2 ox0 - 1, col[r][8] column 2 ox0 + 7; rows 2 oy - 1 .. 2 oy + 1 (only the top row and
// the left column can fall outside an even map).
__device__ __forceinline__ void window_s2(const float* __restrict__ plane, int h, int oy, int ox0,
                                          bool valid, float col[3][9]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int iy = 2 * oy - 1 + r;
        const bool ok = valid && iy >= 0;
        const float* p = plane + iy * h + 2 * ox0;
        const float4 a = ld4(p, ok), b = ld4(p + 4, ok);
        const float l = __shfl_up(b.w, 1, 64);
        col[r][0] = ox0 > 0 ? l : 0.f;
        col[r][1] = a.x; col[r][2] = a.y; col[r][3] = a.z; col[r][4] = a.w;
        col[r][5] = b.x; col[r][6] = b.y; col[r][7] = b.z; col[r][8] = b.w;
    }
}

// ---- forward (and the stride-1 input gradient: the same correlation with the weights
// rotated by 180 degrees, FLIP) ------------------------------------------------------------
template <int STRIDE, bool FLIP>
__global__ void __launch_bounds__(256)
dwconv3x3_kernel(const float* __restrict__ x, int64_t x_cs, const float* __restrict__ w,
                 int64_t w_cs, float* __restrict__ y, int64_t y_cs,
                 const int32_t* __restrict__ counts, int batch, DwGeom g, int accumulate) {
    const int z = blockIdx.y;
    const int cnt = counts ? min(counts[z], batch) : batch;
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;          // float4 of y
    const uint32_t p = e >> g.q4_shift, q = e & ((1u << g.q4_shift) - 1u);
    uint32_t img, c;
    g.divC.divmod(p, img, c);
    const bool valid = img < (uint32_t)cnt;
    const int oy = q >> g.row_shift, ox0 = 4 * (q & ((1u << g.row_shift) - 1u));
    const float* plane = x + z * x_cs + (int64_t)p * (g.h * g.h);
    float wr[9];
    const float* wc = w + z * w_cs + (int64_t)c * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) wr[FLIP ? 8 - i : i] = valid ? wc[i] : 0.f;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (STRIDE == 1) {
        float col[3][6];
        window_s1(plane, g.h, oy, ox0, valid, col);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = fmaf(wr[3 * r + k], col[r][j + k], o[j]);
    } else {
        float col[3][9];
        window_s2(plane, g.h, oy, ox0, valid, col);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = fmaf(wr[3 * r + k], col[r][2 * j + k], o[j]);
    }
    if (!valid) return;  // after the last shuffle
    float4* yp = reinterpret_cast<float4*>(y + z * y_cs + (int64_t)p * (g.ho * g.ho)
                                           + oy * g.ho + ox0);
    float4 r4 = make_float4(o[0], o[1], o[2], o[3]);
    if (accumulate) {
        const float4 old = *yp;
        r4.x += old.x; r4.y += old.y; r4.z += old.z; r4.w += old.w;
    }
    *yp = r4;
}

// ---- stride-2 input gradient -----------------------------------------------------------------
// dX[iy][ix] = sum over (ky, kx) with iy = 2 oy - 1 + ky, ix = 2 ox - 1 + kx of
// dY[oy][ox] w[ky][kx]: an even row takes ky = 1 from dY row iy / 2; an odd row ky = 0 from row
// (iy + 1) / 2 (inside the map) and ky = 2 from row (iy - 1) / 2; columns alike.  A thread owns
// dX (iy, ix0 .. ix0 + 3) and reads dY columns ix0 / 2, + 1 (one float2) and + 2 (the next lane's).
__global__ void __launch_bounds__(256)
dwconv3x3_dgrad_s2_kernel(const float* __restrict__ dy, int64_t dy_cs,
                          const float* __restrict__ w, int64_t w_cs, float* __restrict__ dx,
                          int64_t dx_cs, const int32_t* __restrict__ counts, int batch, DwGeom g,
                          int accumulate) {
    const int z = blockIdx.y;
    const int cnt = counts ? min(counts[z], batch) : batch;
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;          // float4 of dX
    const uint32_t p = e >> g.q4_shift, q = e & ((1u << g.q4_shift) - 1u);
    uint32_t img, c;
    g.divC.divmod(p, img, c);
    const bool valid = img < (uint32_t)cnt;
    const int iy = q >> g.row_shift, ix0 = 4 * (q & ((1u << g.row_shift) - 1u));
    const int ho = g.ho, c0 = ix0 >> 1;
    const float* plane = dy + z * dy_cs + (int64_t)p * (ho * ho);
    float wr[9];
    const float* wc = w + z * w_cs + (int64_t)c * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) wr[i] = valid ? wc[i] : 0.f;
    const bool odd = iy & 1;
    // row A: ky = odd ? 0 : 1; row B (odd rows only): ky = 2
    const int oyA = odd ? (iy + 1) >> 1 : iy >> 1, oyB = (iy - 1) >> 1;
    const bool okA = valid && oyA < ho, okB = valid && odd;
    float wa[3], wb[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        wa[k] = odd ? wr[k] : wr[3 + k];
        wb[k] = wr[6 + k];
    }
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const bool ok = r ? okB : okA;
        const float* rp = plane + (r ? oyB : oyA) * ho + c0;
        const float2 d = ok ? *reinterpret_cast<const float2*>(rp) : make_float2(0.f, 0.f);
        const float nx = __shfl_down(d.x, 1, 64);
        const float d2 = c0 + 2 < ho ? nx : 0.f;
        const float* wk = r ? wb : wa;
        o[0] = fmaf(d.x, wk[1], o[0]);
        o[1] = fmaf(d.y, wk[0], o[1]);
        o[1] = fmaf(d.x, wk[2], o[1]);
        o[2] = fmaf(d.y, wk[1], o[2]);
        o[3] = fmaf(d2, wk[0], o[3]);
        o[3] = fmaf(d.y, wk[2], o[3]);
    }
    if (!valid) return;  // after the last shuffle
    float4* xp = reinterpret_cast<float4*>(dx + z * dx_cs + (int64_t)p * (g.h * g.h)
                                           + iy * g.h + ix0);
    float4 r4 = make_float4(o[0], o[1], o[2], o[3]);
    if (accumulate) {
        const float4 old = *xp;
        r4.x += old.x; r4.y += old.y; r4.z += old.z; r4.w += old.w;
    }
    *xp = r4;
}

// ---- weight gradient -------------------------------------------------------------------------
// One workgroup per (channel, image split, client): dW[c][ky][kx] = sum over the split's valid
// images and the output pixels of dY[oy][ox] x[s oy - 1 + ky][s ox - 1 + kx].  splits == 1
// writes dW, else the split's nine sums go to part [client][C][splits][9].
template <int STRIDE>
__global__ void __launch_bounds__(256)
dwconv3x3_wgrad_kernel(const float* __restrict__ x, int64_t x_cs, const float* __restrict__ dy,
                       int64_t dy_cs, float* __restrict__ dw, int64_t dw_cs,
                       float* __restrict__ part, const int32_t* __restrict__ counts, int batch,
                       DwGeom g, int splits, int per_split) {
    __shared__ float red[4][9];
    const int c = blockIdx.x, s = blockIdx.y, z = blockIdx.z, tid = threadIdx.x;
    const int cnt = counts ? min(counts[z], batch) : batch;
    const int i0 = s * per_split, i1 = min(cnt, i0 + per_split);
    const int total = i1 > i0 ? (i1 - i0) << g.q4_shift : 0;    // float4s of dY, this split
    const int64_t img_x = (int64_t)g.C * g.h * g.h, img_y = (int64_t)g.C * g.ho * g.ho;
    const float* xc = x + z * x_cs + (int64_t)c * (g.h * g.h);
    const float* dc = dy + z * dy_cs + (int64_t)c * (g.ho * g.ho);
    float acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = 0.f;
    for (int e0 = 0; e0 < total; e0 += 256) {   // block-uniform trip count: shuffles inside
        const int e = e0 + tid;
        const bool valid = e < total;
        const int img = i0 + (e >> g.q4_shift), q = e & ((1 << g.q4_shift) - 1);
        const int oy = q >> g.row_shift, ox0 = 4 * (q & ((1 << g.row_shift) - 1));
        const float4 gv = ld4(dc + img * img_y + oy * g.ho + ox0, valid);
        const float gj[4] = {gv.x, gv.y, gv.z, gv.w};
        const float* plane = xc + img * img_x;
        if constexpr (STRIDE == 1) {
            float col[3][6];
            window_s1(plane, g.h, oy, ox0, valid, col);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[3 * r + k] = fmaf(gj[j], col[r][j + k], acc[3 * r + k]);
        } else {
            float col[3][9];
            window_s2(plane, g.h, oy, ox0, valid, col);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[3 * r + k] = fmaf(gj[j], col[r][2 * j + k], acc[3 * r + k]);
        }
    }
    const int lane = tid & 63, wid = tid >> 6;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const float v = wave_sum(acc[i]);
        if (lane == 0) red[wid][i] = v;
    }
    __syncthreads();
    if (tid < 9) {
        const float v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        if (splits == 1)
            dw[z * dw_cs + (int64_t)c * 9 + tid] = v;
        else
            part[(((int64_t)z * g.C + c) * splits + s) * 9 + tid] = v;
    }
}

// dW[client][c][k] = the splits' partials added in split order
__global__ void __launch_bounds__(256)
dwconv3x3_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw,
                              int64_t dw_cs, int n_per_client, int splits) {
    const int z = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;   // i = c * 9 + k
    if (i >= n_per_client) return;
    const int c = i / 9, k = i - 9 * c;
    const float* p = part + ((int64_t)z * n_per_client / 9 + c) * splits * 9 + k;
    float v = 0.f;
    for (int s = 0; s < splits; ++s) v += p[s * 9];
    dw[z * dw_cs + i] = v;
}

int ilog2(int v) {
    int s = 0;
    while ((1 << s) < v) ++s;
    return s;
}

// float4 tiling of the hmap x hmap planes a thread grid covers
DwGeom make_geom(int C, int h, int stride, int hmap) {
    DwGeom g;
    g.C = C;
    g.h = h;
    g.ho = h / stride;
    g.q4_shift = ilog2(hmap * hmap / 4);
    g.row_shift = ilog2(hmap / 4);
    g.divC = FastDiv((uint32_t)C);
    return g;
}

bool aligned16(const void* p, int64_t cs) { return ((uintptr_t)p & 15) == 0 && (cs & 3) == 0; }

int check_shape(const char* fn, int nclients, int batch, int C, int h, int w_, int kh, int kw,
                int stride, int pad) {
    FH_REQUIRE(nclients >= 0 && batch > 0 && C > 0 && h > 0 && w_ > 0, "%s: bad shape", fn);
    if (kh != 3 || kw != 3 || pad != 1 || (stride != 1 && stride != 2) || h != w_ ||
        (h != 8 && h != 16 && h != 32) || C % 8 != 0) {
        set_error("%s: unsupported shape (needs 3x3, pad 1, stride 1|2, square 8/16/32 maps, "
                  "C %% 8 == 0; got k %dx%d pad %d stride %d map %dx%d C %d)", fn, kh, kw, pad,
                  stride, h, w_, C);
        return FH_E_UNSUPPORTED;
    }
    FH_REQUIRE((int64_t)batch * C * h * h < (int64_t)1 << 31, "%s: batch too large", fn);
    FH_REQUIRE(nclients <= 65535, "%s: too many clients (%d > 65535)", fn, nclients);
    return FH_OK;
}

// image splits of the weight gradient: enough workgroups to fill the chip when few clients
// (or channels) are left; a function of the shape alone
int wgrad_splits(int nclients, int batch, int C) {
    const int64_t groups = (int64_t)std::max(nclients, 1) * C;
    const int want = (int)std::min<int64_t>(batch, ceil_div(1024, groups));
    return std::max(want, 1);
}

}  // namespace

}  // namespace fh

using namespace fh;

extern "C" int fh_dwconv3x3_fwd(const float* x, int64_t x_cs, const float* w, int64_t w_cs,
                                float* y, int64_t y_cs, const int32_t* counts, int32_t nclients,
                                int32_t batch, int32_t C, int32_t h, int32_t w_, int32_t kh,
                                int32_t kw, int32_t stride, int32_t pad, void* stream) {
    const int rc = check_shape("dwconv3x3_fwd", nclients, batch, C, h, w_, kh, kw, stride, pad);
    if (rc != FH_OK) return rc;
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(x && w && y, "dwconv3x3_fwd: null pointer");
    if (!aligned16(x, x_cs) || !aligned16(y, y_cs)) {
        set_error("dwconv3x3_fwd: x / y must be 16-byte aligned with client strides %% 4 == 0");
        return FH_E_UNSUPPORTED;
    }
    const int ho = h / stride;
    const DwGeom g = make_geom(C, h, stride, ho);
    const dim3 grid((uint32_t)ceil_div((int64_t)batch * C * ho * ho / 4, 256), nclients);
    if (stride == 1)
        FH_LAUNCH((dwconv3x3_kernel<1, false>), grid, dim3(256), 0, as_stream(stream), x, x_cs, w,
                  w_cs, y, y_cs, counts, batch, g, 0);
    else
        FH_LAUNCH((dwconv3x3_kernel<2, false>), grid, dim3(256), 0, as_stream(stream), x, x_cs, w,
                  w_cs, y, y_cs, counts, batch, g, 0);
    FH_LAUNCH_CHECK("dwconv3x3_fwd");
    return FH_OK;
}

extern "C" int fh_dwconv3x3_dgrad(const float* dy, int64_t dy_cs, const float* w, int64_t w_cs,
                                  float* dx, int64_t dx_cs, const int32_t* counts,
                                  int32_t nclients, int32_t batch, int32_t C, int32_t h,
                                  int32_t w_, int32_t kh, int32_t kw, int32_t stride, int32_t pad,
                                  int32_t accumulate, void* stream) {
    const int rc = check_shape("dwconv3x3_dgrad", nclients, batch, C, h, w_, kh, kw, stride, pad);
    if (rc != FH_OK) return rc;
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(dy && w && dx, "dwconv3x3_dgrad: null pointer");
    if (!aligned16(dy, dy_cs) || !aligned16(dx, dx_cs)) {
        set_error("dwconv3x3_dgrad: dy / dx must be 16-byte aligned with client strides %% 4 == 0");
        return FH_E_UNSUPPORTED;
    }
    const dim3 grid((uint32_t)ceil_div((int64_t)batch * C * h * h / 4, 256), nclients);
    if (stride == 1) {
        // the forward kernel on dY with the weights rotated by 180 degrees
        const DwGeom g = make_geom(C, h, 1, h);
        FH_LAUNCH((dwconv3x3_kernel<1, true>), grid, dim3(256), 0, as_stream(stream), dy, dy_cs, w,
                  w_cs, dx, dx_cs, counts, batch, g, accumulate ? 1 : 0);
    } else {
        const DwGeom g = make_geom(C, h, 2, h);
        FH_LAUNCH(dwconv3x3_dgrad_s2_kernel, grid, dim3(256), 0, as_stream(stream), dy, dy_cs, w,
                  w_cs, dx, dx_cs, counts, batch, g, accumulate ? 1 : 0);
    }
    FH_LAUNCH_CHECK("dwconv3x3_dgrad");
    return FH_OK;
}

extern "C" size_t fh_dwconv3x3_wgrad_workspace(int32_t nclients, int32_t batch, int32_t C,
                                               int32_t h, int32_t w_, int32_t stride) {
    (void)h; (void)w_; (void)stride;
    if (nclients <= 0 || batch <= 0 || C <= 0) return 0;
    const int splits = wgrad_splits(nclients, batch, C);
    return splits > 1 ? (size_t)nclients * C * splits * 9 * sizeof(float) : 0;
}

extern "C" int fh_dwconv3x3_wgrad(const float* x, int64_t x_cs, const float* dy, int64_t dy_cs,
                                  float* dw, int64_t dw_cs, void* workspace, size_t ws_bytes,
                                  const int32_t* counts, int32_t nclients, int32_t batch,
                                  int32_t C, int32_t h, int32_t w_, int32_t kh, int32_t kw,
                                  int32_t stride, int32_t pad, void* stream) {
    const int rc = check_shape("dwconv3x3_wgrad", nclients, batch, C, h, w_, kh, kw, stride, pad);
    if (rc != FH_OK) return rc;
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(x && dy && dw, "dwconv3x3_wgrad: null pointer");
    if (!aligned16(x, x_cs) || !aligned16(dy, dy_cs)) {
        set_error("dwconv3x3_wgrad: x / dy must be 16-byte aligned with client strides %% 4 == 0");
        return FH_E_UNSUPPORTED;
    }
    int splits = wgrad_splits(nclients, batch, C);
    const size_t need = fh_dwconv3x3_wgrad_workspace(nclients, batch, C, h, w_, stride);
    if (splits > 1 && (!workspace || ws_bytes < need)) splits = 1;  // like the conv split plans
    const int per_split = (int)ceil_div(batch, splits);
    splits = (int)ceil_div(batch, per_split);
    const int ho = h / stride;
    const DwGeom g = make_geom(C, h, stride, ho);
    float* part = splits > 1 ? static_cast<float*>(workspace) : nullptr;
    const dim3 grid(C, splits, nclients);
    if (stride == 1)
        FH_LAUNCH(dwconv3x3_wgrad_kernel<1>, grid, dim3(256), 0, as_stream(stream), x, x_cs, dy,
                  dy_cs, dw, dw_cs, part, counts, batch, g, splits, per_split);
    else
        FH_LAUNCH(dwconv3x3_wgrad_kernel<2>, grid, dim3(256), 0, as_stream(stream), x, x_cs, dy,
                  dy_cs, dw, dw_cs, part, counts, batch, g, splits, per_split);
    if (splits > 1)
        FH_LAUNCH(dwconv3x3_wgrad_reduce_kernel, dim3((uint32_t)ceil_div(C * 9, 256), nclients),
                  dim3(256), 0, as_stream(stream), part, dw, dw_cs, C * 9, splits);
    FH_LAUNCH_CHECK("dwconv3x3_wgrad");
    return FH_OK;
}
