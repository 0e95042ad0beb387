// dconv_kernels.h — direct 3x3 / stride 1 / pad 1 convolution on fp32 MFMA, input
// patch staged once in LDS (included by conv.hip: one translation unit).
//
// The generic implicit GEMM (igemm_kernel) gathers every im2col element from
// global memory: 9 loads and their address arithmetic per input value, which
// on the CIFAR layers costs as many VALU cycles as the MFMAs it feeds.  Here a
// workgroup owns 256 consecutive output pixels (TR whole rows of width W, one
// image or several small ones) x BM output channels and stages, per chunk of
// CK reduction channels,
//   * the input rows its pixels touch, with a zero halo, once:
//       Ps[ch][patch_row][W+2]      (the 3x3 shifts become LDS address offsets)
//   * the weights as As[(kh*3+kw)*CK + ch][m]
// so one staged value feeds up to 9 MFMA operands and the inner loop is pure
// ds_read_b32 (compile-time immediates) + v_mfma_f32_32x32x2_f32.
// The K order pairs channels (ch, ch+1) at the same (kh,kw), so the two
// k-values one MFMA consumes (lanes 0-31 / 32-63) sit exactly one channel
// stride apart in both images.
//
//   FWD   : Y[m][pix]  = sum_{ch,kh,kw} W[m][ch][kh][kw]     X[ch][pix + (kh-1, kw-1)]
//   DGRAD : dX[m][pix] = sum_{ch,kh,kw} W[ch][m][2-kh][2-kw] dY[ch][pix + (kh-1, kw-1)]
// (dgrad of a stride-1 pad-1 3x3 conv is the same stencil on dY with the
// weights transposed and flipped).
#pragma once

namespace fh {

// Pooled output gradient (r05, SimpleCNN conv2's backward; fh_conv_pooled_dy): the layer's
// output gradient is not materialised.  Pixel (y, x) of a plane takes the following 2x2
// max-pool's gradient g[y/2][x/2] (dense pooled planes ph x ph) when (y, x) is its window's
// argmax idx and the pooled ReLU output yp there is > 0, else 0 — fh_maxpool2_bwd_ymask's values
// bit for bit, with rows / columns past the 2ph x 2ph map zero (the plane's zero ring).
struct PooledDy {
    const float* g;      // [z][img][C][ph][ph]
    const uint8_t* idx;  // same layout
    const float* yp;     // same layout
    int64_t g_cs, i_cs, y_cs;
    int ph;
};
// raw loads of a quad (y, x0 .. x0 + 3), x0 % 4 == 0: two pooled gradients, two pooled outputs,
// two argmax bytes | the row parity (routed in pdy_route, after the loads have landed)
__device__ __forceinline__ void pdy_load(const PooledDy& q, int z, int64_t plane, int y, int x0,
                                         bool ok, float2& g, float2& yp, int& code) {
    const int py = y >> 1, px = x0 >> 1;
    const bool r_ok = ok && py < q.ph;
    const bool c0 = r_ok && px < q.ph, c1 = r_ok && px + 1 < q.ph;
    const int64_t e = (plane * q.ph + py) * q.ph + px;
    // in-bounds addresses (element 0 of the client for a dead operand), selects after: r05 —
    // each conditional argmax byte had sat in a branch with its use, one round trip per byte
    const int64_t e0 = c0 ? e : 0, e1 = c1 ? e + 1 : 0;
    const float g0 = q.g[z * q.g_cs + e0], g1 = q.g[z * q.g_cs + e1];
    const float y0 = q.yp[z * q.y_cs + e0], y1 = q.yp[z * q.y_cs + e1];
    const int i0 = q.idx[z * q.i_cs + e0], i1 = q.idx[z * q.i_cs + e1];
    g = make_float2(c0 ? g0 : 0.f, c1 ? g1 : 0.f);
    yp = make_float2(c0 ? y0 : 0.f, c1 ? y1 : 0.f);
    code = (c0 ? i0 : 0) | ((c1 ? i1 : 0) << 8) | ((y & 1) << 17);
}
__device__ __forceinline__ float4 pdy_route(float2 g, float2 yp, int code) {
    const int r = code >> 16, i0 = code & 0xff, i1 = (code >> 8) & 0xff;
    const float g0 = yp.x > 0.f ? g.x : 0.f, g1 = yp.y > 0.f ? g.y : 0.f;
    return make_float4(i0 == r ? g0 : 0.f, i0 == (r | 1) ? g0 : 0.f, i1 == r ? g1 : 0.f,
                       i1 == (r | 1) ? g1 : 0.f);
}

struct DConvArgs {
    const float* in;   // X (FWD) or dY (DGRAD): [client][img][Cr][H][W]
    const float* wt;   // [client] W[cout][cin][3][3]
    const float* bias;
    float* out;        // [client][img][M][H][W], or the split-K slab
    int64_t in_cs, w_cs, b_cs, out_cs;
    const int32_t* counts;
    int batch, Cr, M;  // Cr: reduction channels; M: output channels
    int relu, accumulate;
    int splits, cchunk;  // reduction channels per split (multiple of CK)
    int Nfull;           // batch * H * W (slab row length)
    int wvec;            // host: weight slices 16-B aligned -> float4 staging instance
    // FWD only, nullable: the input is a BatchNorm's pre-activation and the kernel stages
    // relu(x * in_scale[z][c] + in_shift[z][c]) — the BN apply + ReLU done on load
    const float* in_scale;
    const float* in_shift;
    int64_t aff_cs;
    // FWD only, nullable: BatchNorm statistics of the stored output, taken from the
    // accumulators instead of a second pass over y: one fp64 (sum, sum of squares) pair per
    // (client, channel, 256-pixel tile) -> bn_part[((z * M + m) * bn_tiles + t) * 2]
    // (tiles past the client's count hold zeros).  Unsplit launches only; with split-K the
    // epilogue kernel takes the statistics (conv.hip splitk_epilogue_kernel).
    double* bn_part;
    int bn_tiles;
    // DGRAD with bn_part: BatchNorm BACKWARD statistics of the stored gradient.  The conv's
    // input was relu(BN(bnx)); the kernel stores g = (bnx*bn_scale + bn_shift > 0) ? v : 0
    // (the ReLU mask, bn.hip ReluMask) and writes per (client, channel, tile) the fp64 pair
    // (sum g, sum (bnx - bn_mean) g) that bn_bwd_reduce_kernel would take from a second pass.
    const float* bnx;
    int64_t bnx_cs;
    const float* bn_scale;
    const float* bn_shift;
    int64_t bns_cs;
    const float* bn_mean;  // [client][M]
    // ... and pidx non-null: a 2x2 max-pool (+ dropout) sat between that ReLU and this conv
    // (bnx is the full-resolution map, 2H x 2W).  dX is stored as is (the pool's output
    // gradient); the statistics route it as maxpool2_bwd does: to the window argmax
    // pidx (== (y&1)*2 + (x&1)), times the keep-mask pmask / (1 - p) when pmask is non-null.
    const uint8_t* pidx;
    const uint8_t* pmask;
    int64_t pi_cs, pm_cs;
    float pscale;
    // dconv_dgrad_s2_kernel<SC>: the ResNet projection shortcut's 1x1 / stride-2 DGRAD folded
    // in — dX[m][2r][2c] += sum_ch wt2[ch][m] in2[ch][r][c] (in2 = its output gradient)
    const float* in2;
    const float* wt2;
    int64_t in2_cs, w2_cs;
    // FWD, statistics-epilogue instance, unsplit, nullable: a 2x2 max-pool of the ReLU output's
    // top-left pool_hw x pool_hw map (SimpleCNN's 14x14 conv2 on 16x16 planes), taken from the
    // tile's image in LDS with maxpool2_fwd_kernel's first-max rule -> pool_y
    // [img][M][pool_hw/2][pool_hw/2] and the argmax pool_idx (same layout); out is not written
    float* pool_y;
    uint8_t* pool_idx;
    int64_t py_cs, pix_cs;
    int pool_hw;
    // DGRAD, the PDY instances: dY routed from a 2x2 max-pool's gradient (in is not read)
    PooledDy pdy;
};

// Pitch of the [BM channels][256 pixels] fp32 image the statistics pass reduces: 264 = 8
// mod 64, so the epilogue's writes (32 pixels x 2 channel halves 4 apart) hit 64 distinct
// banks and the per-channel strided reads at most 2-way conflicts.
constexpr int kStatPitch = 264;

// BatchNorm apply + ReLU on a staged float4 of channel c (bn.hip bn_apply_kernel's exact
// fp32 operations: x * alpha + beta', then max(., 0); contraction is off in this build)
__device__ __forceinline__ float4 bn_relu4(float4 v, float s, float t) {
    v.x = fmaxf(v.x * s + t, 0.f);
    v.y = fmaxf(v.y * s + t, 0.f);
    v.z = fmaxf(v.z * s + t, 0.f);
    v.w = fmaxf(v.w * s + t, 0.f);
    return v;
}

// Workgroup coordinates.  (r02 measured an XCD-aware remap of this order — each XCD a
// contiguous range so one client's tiles share an L2 — neutral on these MFMA-bound kernels,
// KT 265.6k vs 266.3k, profiles/r02_s3/xcd_ab.txt; removed in r03.)
__device__ __forceinline__ void block_xyz(int& bx, int& by, int& bz) {
    bx = blockIdx.x;
    by = blockIdx.y;
    bz = blockIdx.z;
}

template <int W>
struct DGeom {
    static constexpr int H = W;                       // square images (CIFAR 32/16/8)
    static constexpr int HW = H * W;
    static constexpr int TR = 256 / W;                // output rows per tile
    static constexpr int SEGR = TR < H ? TR : H;      // rows per image segment in a tile
    static constexpr int NI = TR / SEGR;              // image segments per tile
    static constexpr int PW = W + 2;                  // patch row pitch
    static constexpr int PR = NI * (SEGR + 2);        // patch rows
    static constexpr int CSTR = PR * PW;              // patch channel stride
    static_assert(256 % W == 0 && (TR % H == 0 || H % TR == 0), "tile geometry");
};

// S = 2 (FWD only): the 3x3 / stride-2 / pad-1 convolution of the ResNet down-sampling
// blocks (models_pytorch.py:176-181) on the same machinery: the tile is 256 OUTPUT pixels
// (W = output width), the staged patch covers the 2*SEGR+1 input rows those pixels read
// (2W + 2 columns with the halo), and a lane's operand address strides by 2 — the 3x3
// shifts stay LDS immediates.  The channel stride of the patch is odd, so the two lane
// halves (channel pair) fall on opposite bank parities.
// BNB: the instance with the statistics epilogue — FWD the BatchNorm statistics, DGRAD the
// BN-backward statistics (its registers would otherwise cost every instance an occupancy
// step, e.g. DGRAD W=32 BM=32: 96 -> 114 VGPRs, 4 -> 3 waves per SIMD)
// BM = 64: two waves per SIMD (the W=8 FWD statistics instance needed 260 registers, one
// wave per SIMD; its 68 KB of LDS fit two workgroups per CU)
// LDS floats of one dconv workgroup (the stage buffers, or the statistics image when larger)
template <int OP, int W, int BM, int CK, int S, bool BNB>
constexpr int dconv_lds_floats() {
    using G = DGeom<W>;
    constexpr int PRS = S == 1 ? G::SEGR + 2 : 2 * G::SEGR + 1;
    constexpr int PW = S * W + 2, PR = G::NI * PRS;
    constexpr int CSTR = S == 1 ? PR * PW : ((PR * PW) | 1);
    constexpr int MAIN = 2 * 9 * CK * (BM + 1) + 2 * CK * CSTR;
    constexpr int STAT = !BNB ? 0 : BM * kStatPitch + (OP == OP_DGRAD ? 3 * BM : 0);
    return STAT > MAIN ? STAT : MAIN;
}

// the workgroup body; smem holds dconv_lds_floats() floats (dconv_kernel's own array, or
// the array a dual-role launch shares with a WGRAD body: dconv_wgrad_dual_kernel)
template <int OP, int W, int BM, int WAVES_M, int CK, bool WVEC, int S = 1, bool BNB = false,
          bool PDY = false>
__device__ __forceinline__ void dconv_body(const DConvArgs& a, float* smem, int bx, int by,
                                           int bz) {
    using G = DGeom<W>;
    static_assert(!PDY || (OP == OP_DGRAD && S == 1 && W % 4 == 0), "pooled dY: DGRAD");
    static_assert(S == 1 || (S == 2 && OP == OP_FWD), "stride 2: forward only");
    static_assert(!BNB || S == 1, "statistics epilogue: stride 1");
    constexpr int WI = S * W, HI = S * G::H;               // input map
    constexpr int PRS = S == 1 ? G::SEGR + 2 : 2 * G::SEGR + 1;  // input rows per segment
    constexpr int PW = WI + 2, PR = G::NI * PRS;
    constexpr int CSTR = S == 1 ? PR * PW : ((PR * PW) | 1);
    constexpr int WAVES_N = 4 / WAVES_M;
    constexpr int WM = BM / WAVES_M, WN = 256 / WAVES_N;
    constexpr int FM = WM / 32, FN = WN / 32;
    constexpr int BMP = BM + 1;                 // As row pitch (staging writes spread banks)
    constexpr int KS = 9 * CK;                  // k-values per stage
    constexpr int PE = CK * CSTR;               // patch elements per stage
    // staging: patch interior rows as float4 (halo columns are constant zeros), weights
    // as float4 runs of the contiguous [ch][3][3] (FWD) / [m][3][3] (DGRAD) slices
    constexpr int PQ = WI / 4, RPI = 256 / PQ, NPR = CK * PR, NPT = (NPR + RPI - 1) / RPI;
    constexpr int NAV = (BM * KS / 4 + 255) / 256;   // float4 weight slots per thread
    static_assert(FM >= 1 && FN >= 1 && (CK % 2) == 0, "dconv tile");

    // one LDS block: the double-buffered weight / patch stages, reused after the K loop as
    // the statistics image (with bn_part)
    constexpr int LDS_MAIN = 2 * KS * BMP + 2 * PE;
    constexpr int LDS_STAT = !BNB ? 0 : BM * kStatPitch + (OP == OP_DGRAD ? 3 * BM : 0);
    constexpr int LDS_N = LDS_STAT > LDS_MAIN ? LDS_STAT : LDS_MAIN;
    static_assert(LDS_N == dconv_lds_floats<OP, W, BM, CK, S, BNB>(), "dconv LDS size");
    float (*As)[KS * BMP] = reinterpret_cast<float (*)[KS * BMP]>(smem);
    float (*Ps)[PE] = reinterpret_cast<float (*)[PE]>(smem + 2 * KS * BMP);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid / WAVES_N, wn = wid % WAVES_N;
    const int z = bz / a.splits;
    const int split = bz - z * a.splits;
    const int cnt = a.counts ? a.counts[z] : a.batch;
    const int t = bx, m0 = by * BM;
    const int n0 = t * 256;
    // block-uniform: BN statistics of the stored values (FWD) / BN backward statistics of
    // the stored gradient (DGRAD)
    const bool stats = BNB && a.bn_part != nullptr && a.splits == 1;
    // the pooled epilogue's [BM][kStatPitch] image fits in the K loop's LDS (the plain
    // instance: BM = 32) or in the statistics image (the BNB instance)
    constexpr bool POOL_LDS = BNB || LDS_MAIN >= BM * kStatPitch;
    const bool pooled = POOL_LDS && OP == OP_FWD && a.pool_y != nullptr && a.splits == 1;
    if (n0 >= cnt * G::HW) {  // a tile past this client's images: zero statistics
        if (stats && tid < BM && m0 + tid < a.M) {
            double* q = a.bn_part + (((int64_t)z * a.M + m0 + tid) * a.bn_tiles + t) * 2;
            q[0] = 0.0;
            q[1] = 0.0;
        }
        return;
    }
    const int cbeg = split * a.cchunk;
    const int cend = min(a.Cr, cbeg + a.cchunk);
    const int M = a.M;

    for (int q = tid; q < 2 * NPR; q += 256) {  // zero halo columns of both buffers
        const int bsel = q / NPR, row = q % NPR;
        float* r = &Ps[bsel][(row / PR) * CSTR + (row % PR) * PW];
        r[0] = 0.f;
        r[WI + 1] = 0.f;
    }

    const int img0 = (t * G::TR) / G::H, y0 = (t * G::TR) % G::H;
    const int prt = tid / PQ, px = (tid % PQ) * 4;
    const float* inz = a.in + z * a.in_cs;
    const float* wz = a.wt + z * a.w_cs;
    constexpr bool wvec = WVEC;  // scalar weight staging (costly in VGPRs) only when needed

    float4 rp[NPT], ra[NAV];
    float bsc[NPT], bsh[NPT];  // BN affine of each staged row (in_scale set)
    float2 pg[PDY ? NPT : 1], pp[PDY ? NPT : 1];  // PDY: raw pooled loads, routed in store()
    int pc[PDY ? NPT : 1];
    auto load = [&](int c0) {
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int q = prt + i * RPI;
            const int cl = q / PR, pr = q % PR;
            const int seg = pr / PRS, rr = pr % PRS;
            const int img = img0 + seg, y = S * y0 + rr - 1;
            const bool ok = q < NPR && img < cnt && (unsigned)y < (unsigned)HI && c0 + cl < cend;
            if constexpr (PDY) {
                pdy_load(a.pdy, z, (int64_t)img * a.Cr + c0 + cl, y, px, ok, pg[i], pp[i], pc[i]);
                continue;
            }
            rp[i] = ok ? *reinterpret_cast<const float4*>(
                             inz + ((int64_t)(img * a.Cr + c0 + cl) * HI + y) * WI + px)
                       : make_float4(0.f, 0.f, 0.f, 0.f);
            if (OP == OP_FWD && a.in_scale != nullptr) {  // applied in store(): the loads
                bsc[i] = ok ? a.in_scale[z * a.aff_cs + c0 + cl] : 1.f;  // stay in flight over
                bsh[i] = ok ? a.in_shift[z * a.aff_cs + c0 + cl] : 0.f;  // the MFMA loop;
            }                                                // padding: relu(0*1+0) = 0
        }
        if constexpr (wvec) {
#pragma unroll
            for (int i = 0; i < NAV; ++i) {
                const int f = tid + i * 256;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (OP == OP_FWD) {  // run of 9*CK floats per m: W[m0+m][c0 .. c0+CK)[9]
                    const int m = f / (KS / 4), j4 = f % (KS / 4);
                    if (f < BM * KS / 4 && m0 + m < M)
                        v = *reinterpret_cast<const float4*>(
                            wz + ((int64_t)(m0 + m) * a.Cr + c0) * 9 + 4 * j4);
                } else {             // run of 9*BM floats per ch: W[c0+cl][m0 .. m0+BM)[9]
                    const int cl = f / (BM * 9 / 4), j4 = f % (BM * 9 / 4);
                    if (f < BM * KS / 4 && c0 + cl < cend)
                        v = *reinterpret_cast<const float4*>(
                            wz + ((int64_t)(c0 + cl) * M + m0) * 9 + 4 * j4);
                }
                ra[i] = v;
            }
        } else {
            float* rs = reinterpret_cast<float*>(ra);
#pragma unroll
            for (int i = 0; i < 4 * NAV; ++i) {
                const int e = tid + i * 256;
                float v = 0.f;
                if (OP == OP_FWD) {
                    const int m = e / KS, rem = e % KS, cl = rem / 9, r9 = rem % 9;
                    if (e < BM * KS && m0 + m < M && c0 + cl < cend)
                        v = wz[((int64_t)(m0 + m) * a.Cr + c0 + cl) * 9 + r9];
                } else {
                    const int cl = e / (BM * 9), rem = e % (BM * 9), m = rem / 9, r9 = rem % 9;
                    if (e < BM * KS && m0 + m < M && c0 + cl < cend)
                        v = wz[((int64_t)(c0 + cl) * M + m0 + m) * 9 + (8 - r9)];
                }
                rs[i] = v;
            }
        }
    };
    // As[(r9*CK + cl)*BMP + m]; r9 is the patch shift (kh*3+kw) the weight multiplies
    auto put_a = [&](int buf, int m, int cl, int r9, float v, int c0) {
        if (m0 + m >= M || c0 + cl >= cend) v = 0.f;
        As[buf][(r9 * CK + cl) * BMP + m] = v;
    };
    auto store = [&](int buf, int c0) {
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int q = prt + i * RPI;
            if (q < NPR) {
                if constexpr (PDY) rp[i] = pdy_route(pg[i], pp[i], pc[i]);
                if (OP == OP_FWD && a.in_scale != nullptr) rp[i] = bn_relu4(rp[i], bsc[i], bsh[i]);
                float* d = &Ps[buf][(q / PR) * CSTR + (q % PR) * PW + 1 + px];
                d[0] = rp[i].x;
                d[1] = rp[i].y;
                d[2] = rp[i].z;
                d[3] = rp[i].w;
            }
        }
        if constexpr (wvec) {
#pragma unroll
            for (int i = 0; i < NAV; ++i) {
                const int f = tid + i * 256;
                if (f < BM * KS / 4) {
                    const float vv[4] = {ra[i].x, ra[i].y, ra[i].z, ra[i].w};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (OP == OP_FWD) {
                            const int m = f / (KS / 4), k = 4 * (f % (KS / 4)) + u;
                            put_a(buf, m, k / 9, k % 9, vv[u], c0);
                        } else {
                            const int cl = f / (BM * 9 / 4), k = 4 * (f % (BM * 9 / 4)) + u;
                            put_a(buf, k / 9, cl, 8 - k % 9, vv[u], c0);
                        }
                    }
                }
            }
        } else {
            const float* rs = reinterpret_cast<const float*>(ra);
#pragma unroll
            for (int i = 0; i < 4 * NAV; ++i) {
                const int e = tid + i * 256;
                if (e < BM * KS) {
                    if (OP == OP_FWD) {
                        const int rem = e % KS;
                        put_a(buf, e / KS, rem / 9, rem % 9, rs[i], c0);
                    } else {
                        const int rem = e % (BM * 9);
                        put_a(buf, rem / 9, e / (BM * 9), rem % 9, rs[i], c0);
                    }
                }
            }
        }
    };

    f32x16 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // lane operand bases: half h = lane>>5 takes the odd channel of each pair
    const int h = lane >> 5, col = lane & 31;
    const int a_lane = h * BMP + wm * WM + col;
    int b_lane[FN];
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int n = wn * WN + j * 32 + col;  // local pixel
        const int ir = n / W, c = n % W;
        const int seg = ir / G::SEGR, lr = ir % G::SEGR;
        b_lane[j] = h * CSTR + (seg * PRS + S * lr) * PW + S * c;
    }

    // r05: live map rows.  SimpleCNN's conv2 runs its 14x14 map on zero-ringed 16x16 planes;
    // the pooled forward (pool_y set) and the pooled-dY DGRAD read / write only the map's rows,
    // so the output block of rows 14-15 (the last 32-pixel block of a one-image W = 16 tile) is
    // never read: the wave owning it skips that block's operand reads and MFMAs (its
    // accumulator stays zero; every live block's MFMA chain is unchanged, the same bits).
    int live_h = G::H;
    if constexpr (W == 16 && S == 1 && G::NI == 1) {
        if (OP == OP_FWD && a.pool_y != nullptr) live_h = a.pool_hw;
        if constexpr (PDY) live_h = 2 * a.pdy.ph;
    }
    const bool skip_last = W == 16 && (wn * WN + (FN - 1) * 32) / W >= live_h;  // wave-uniform

    auto kloop = [&](auto nl_c) {
        constexpr int NL = decltype(nl_c)::value;  // live 32-pixel blocks of this wave
        load(cbeg);
        store(0, cbeg);
        __syncthreads();
        int buf = 0;
        for (int c0 = cbeg; c0 < cend; c0 += CK) {
            const bool more = c0 + CK < cend;
            if (more) load(c0 + CK);
            // kh rolled (bounds the compiler's LDS-read hoisting, i.e. VGPRs); the 3*CK/2
            // (kw, channel-pair) items of a kh are unrolled with every operand offset a
            // ds_read immediate, and operands are double-buffered in registers: item j+1
            // is read while item j's MFMAs issue.
            constexpr int NI = 3 * (CK / 2);
#pragma unroll 1
            for (int kh = 0; kh < 3; ++kh) {
                const float* Ab = &As[buf][a_lane + kh * 3 * CK * BMP];
                const float* Pb = &Ps[buf][kh * PW];
                float av[2][FM], bv[2][FN];
                auto fetch = [&](int j, int slot) {
                    const int kw = j / (CK / 2), cp = j % (CK / 2);
#pragma unroll
                    for (int i = 0; i < FM; ++i)
                        av[slot][i] = Ab[(kw * CK + 2 * cp) * BMP + i * 32];
#pragma unroll
                    for (int jj = 0; jj < NL; ++jj)
                        bv[slot][jj] = Pb[b_lane[jj] + 2 * cp * CSTR + kw];
                };
                fetch(0, 0);
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    if (j + 1 < NI) fetch(j + 1, (j + 1) & 1);
#pragma unroll
                    for (int i = 0; i < FM; ++i)
#pragma unroll
                        for (int jj = 0; jj < NL; ++jj)
                            acc[i][jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                                av[j & 1][i], bv[j & 1][jj], acc[i][jj], 0, 0, 0);
                    // schedule: the next item's operand reads (DS read group), then this item's
                    // MFMAs — one group per item, so each wait covers only the reads issued an
                    // item earlier (r04: the compiler had paired items and waited on fresh reads;
                    // per launch 1-4 %, the 8x8 FWD at 23 clients 16 %, profiles/r04_h/)
                    if (j + 1 < NI) __builtin_amdgcn_sched_group_barrier(0x100, FM + NL, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, FM * NL, 0);
                }
            }
            if (more) store(buf ^ 1, c0 + CK);
            __syncthreads();
            buf ^= 1;
        }
    };
    if (cbeg < cend) {
        if constexpr (W == 16 && FN > 1) {
            if (skip_last) kloop(std::integral_constant<int, FN - 1>{});
            else kloop(std::integral_constant<int, FN>{});
        } else {
            kloop(std::integral_constant<int, FN>{});
        }
    }

    // ---- epilogue: lanes = 32 consecutive pixels -> coalesced stores ----
    const int rbase = 4 * h;
    if constexpr (BNB && OP == OP_DGRAD) {
        if (stats) {  // BN backward statistics (host: no accumulate)
            float* red = smem;                         // [BM][kStatPitch] image
            float* cst = smem + BM * kStatPitch;       // [3][BM] scale, shift, mean
            if (tid < BM) {
                const int m = m0 + tid;
                const bool ok = m < M;
                cst[tid] = ok ? a.bn_scale[z * a.bns_cs + m] : 0.f;
                cst[BM + tid] = ok ? a.bn_shift[z * a.bns_cs + m] : 0.f;
                cst[2 * BM + tid] = ok ? a.bn_mean[z * M + m] : 0.f;
            }
            __syncthreads();
            // pass 1: g = ReLU-masked dX (routed through the pool when pidx), imaged; acc
            // keeps (x - mean) * g, the fp32 product bn_bwd_reduce_kernel promotes
            const bool pooled = a.pidx != nullptr;
#pragma unroll
            for (int j = 0; j < FN; ++j) {
                const int n = n0 + wn * WN + j * 32 + col;
                const int img = n / G::HW, p = n % G::HW;
                const bool live = img < cnt;
                float* op = a.out + z * a.out_cs + (int64_t)img * M * G::HW + p;
                float xv[FM][16];  // all loads of the column first: `out` may alias `bnx`
                int cd[FM][16];    // pooled: argmax (bits 0-1) | kept (bit 2)
                if (pooled) {
                    // argmax and keep-mask bytes of the column loaded from in-bounds addresses
                    // (dead elements read element 0; a null keep-mask reads the argmax bytes)
                    // and combined after: r05 — the keep-mask test had put each element's load
                    // and use in a branch of its own, one dependent round trip per element
                    const int64_t e0 = (int64_t)img * M * G::HW + p;
                    const uint8_t* pi = a.pidx + z * a.pi_cs;
                    const uint8_t* pk = a.pmask ? a.pmask + z * a.pm_cs : pi;
                    uint32_t ib[FM][16], kb[FM][16];
#pragma unroll
                    for (int i = 0; i < FM; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int m = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + rbase;
                            const int64_t e = (live && m < M) ? e0 + (int64_t)m * G::HW : 0;
                            ib[i][r] = pi[e];
                            kb[i][r] = pk[e];
                        }
#pragma unroll
                    for (int i = 0; i < FM; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int m = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + rbase;
                            cd[i][r] = (live && m < M)
                                           ? (int)ib[i][r] | ((!a.pmask || kb[i][r]) ? 4 : 0)
                                           : 0;
                        }
                    const int py = p / G::H, px = p % G::H;
                    const float* xz = a.bnx + z * a.bnx_cs + (int64_t)img * M * 4 * G::HW +
                                      (2 * py) * (2 * G::H) + 2 * px;
#pragma unroll
                    for (int i = 0; i < FM; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int m = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + rbase;
                            const int code = cd[i][r];
                            xv[i][r] = (live && m < M)
                                           ? xz[(int64_t)m * 4 * G::HW + (code >> 1 & 1) * 2 * G::H +
                                                (code & 1)]
                                           : 0.f;
                        }
                } else {
                    const float* xz = a.bnx + z * a.bnx_cs + (int64_t)img * M * G::HW + p;
#pragma unroll
                    for (int i = 0; i < FM; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int m = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + rbase;
                            xv[i][r] = (live && m < M) ? xz[(int64_t)m * G::HW] : 0.f;
                            cd[i][r] = 4;
                        }
                }
#pragma unroll
                for (int i = 0; i < FM; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int ml = wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + rbase;
                        const int m = m0 + ml;
                        float g = 0.f, pv = 0.f;
                        if (live && m < M) {
                            const float v = acc[i][j][r];
                            float gu = v;  // the gradient reaching the BN-ReLU output element
                            if (pooled) gu = !(cd[i][r] & 4) ? 0.f : a.pmask ? v * a.pscale : v;
                            g = (xv[i][r] * cst[ml] + cst[BM + ml] > 0.f) ? gu : 0.f;
                            pv = (xv[i][r] - cst[2 * BM + ml]) * g;
                            op[(int64_t)m * G::HW] = pooled ? v : g;
                        }
                        red[ml * kStatPitch + n - n0] = g;
                        acc[i][j][r] = pv;
                    }
            }
            constexpr int TPC = 256 / BM;
            const int c = tid / TPC, q = tid % TPC;
            auto image_sum = [&]() {  // per channel: TPC threads, fixed order, fp64
                double s0 = 0.0;
#pragma unroll 8
                for (int k = 0; k < 256 / TPC; ++k) s0 += (double)red[c * kStatPitch + q + TPC * k];
#pragma unroll
                for (int o = 1; o < TPC; o <<= 1) s0 += __shfl_xor(s0, o, 64);
                return s0;
            };
            __syncthreads();
            const double sg = image_sum();
            __syncthreads();
#pragma unroll
            for (int j = 0; j < FN; ++j)
#pragma unroll
                for (int i = 0; i < FM; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        red[(wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + rbase) * kStatPitch +
                            wn * WN + j * 32 + col] = acc[i][j][r];
            __syncthreads();
            const double dot = image_sum();
            const int m = m0 + c;
            if (q == 0 && m < M) {
                double* d = a.bn_part + (((int64_t)z * M + m) * a.bn_tiles + t) * 2;
                d[0] = sg;
                d[1] = dot;
            }
            return;
        }
    }
    // the bias of this lane's 16*FM output channels, read once into registers (inside the
    // store loop the compiler must re-read it after every store: `out` may alias `bias`)
    float bv_r[FM][16];
    if (OP == OP_FWD && a.splits == 1) {
        const float* bz = a.bias ? a.bias + z * a.b_cs : nullptr;
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + rbase;
                bv_r[i][r] = (bz && m < M) ? bz[m] : 0.f;
            }
    }
    // statistics image (FWD with bn_part): the stored value of every (channel, pixel) of
    // the tile, [BM][kStatPitch] fp32 in the LDS the K loop has finished with
    float* red = smem;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int n = n0 + wn * WN + j * 32 + col;
        const int img = n / G::HW, p = n % G::HW;
        if (img >= cnt) {
            if (stats) {  // past the client's images: contributes zero
#pragma unroll
                for (int i = 0; i < FM; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        red[(wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + rbase) * kStatPitch +
                            n - n0] = 0.f;
            }
            continue;
        }
        if (a.splits > 1) {
            float* op = a.out + ((int64_t)bz * M) * a.Nfull + n;
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + rbase;
                    if (m < M) op[(int64_t)m * a.Nfull] = acc[i][j][r];
                }
        } else {
            float* op = a.out + z * a.out_cs + (int64_t)img * M * G::HW + p;
            const bool has_bias = a.bias != nullptr;
            // DGRAD accumulating onto dX (a ResNet block's conv1 onto the shortcut gradient):
            // each 16-row group's old values loaded first (r05: read under the branch, each
            // element's read-modify-write was one dependent round trip)
#pragma unroll
            for (int i = 0; i < FM; ++i) {
                float old[16];
                if (OP == OP_DGRAD && a.accumulate) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + rbase;
                        old[r] = op[(int64_t)(m < M ? m : 0) * G::HW];
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ml = wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + rbase;
                    const int m = m0 + ml;
                    if (m < M) {
                        float v = acc[i][j][r];
                        float* q = op + (int64_t)m * G::HW;
                        if (OP == OP_FWD) {
                            if (has_bias) v = v + bv_r[i][r];
                            if (a.relu) v = fmaxf(v, 0.f);
                            if (stats || pooled) red[ml * kStatPitch + n - n0] = v;
                            if (pooled) continue;  // only the pooled map leaves the tile
                        } else if (a.accumulate) {
                            v = old[r] + v;
                        }
                        *q = v;
                    }
                }
            }
        }
    }
    if constexpr (OP == OP_FWD && POOL_LDS && G::HW <= 256) {
        if (pooled) {  // 2x2 max-pool of each whole image of the tile, from the LDS image
            __syncthreads();
            constexpr int IMGS = 256 / G::HW;
            const int ph = a.pool_hw >> 1, per = ph * ph;
            const int img_t = n0 / G::HW;
            for (int e = tid; e < BM * IMGS * per; e += 256) {
                const int ml = e / (IMGS * per), rem = e - ml * (IMGS * per);
                const int li = rem / per, pp = rem - li * per;
                const int oy = pp / ph, ox = pp - oy * ph;
                const int m = m0 + ml, img = img_t + li;
                if (m >= M || img >= cnt) continue;
                const float* r = red + ml * kStatPitch + li * G::HW + (2 * oy) * W + 2 * ox;
                const float v0 = r[0], v1 = r[1], v2 = r[W], v3 = r[W + 1];
                float mx = v0;
                int am = 0;
                if (v1 > mx) { mx = v1; am = 1; }
                if (v2 > mx) { mx = v2; am = 2; }
                if (v3 > mx) { mx = v3; am = 3; }
                const int64_t o = ((int64_t)img * M + m) * per + pp;
                a.pool_y[z * a.py_cs + o] = mx;
                a.pool_idx[z * a.pix_cs + o] = (uint8_t)am;
            }
        }
    }
    if constexpr (OP == OP_FWD) {
        if (stats) {
            // BatchNorm statistics of the tile's stored values per output channel, in a
            // fixed order: TPC threads per channel each add 256/TPC pixels (stride TPC) in
            // fp64 (x and x*x, as bn_stats_kernel), then combine by xor-shuffles.
            constexpr int TPC = 256 / BM;
            __syncthreads();
            const int c = tid / TPC, q = tid % TPC;
            double s0 = 0.0, s1 = 0.0;
#pragma unroll 8
            for (int k = 0; k < 256 / TPC; ++k) {
                const double v = red[c * kStatPitch + q + TPC * k];
                s0 += v;
                s1 += v * v;
            }
#pragma unroll
            for (int o = 1; o < TPC; o <<= 1) {
                s0 += __shfl_xor(s0, o, 64);
                s1 += __shfl_xor(s1, o, 64);
            }
            const int m = m0 + c;
            if (q == 0 && m < M) {
                double* d = a.bn_part + (((int64_t)z * M + m) * a.bn_tiles + t) * 2;
                d[0] = s0;
                d[1] = s1;
            }
        }
    }
}

template <int OP, int W, int BM, int WAVES_M, int CK, bool WVEC, int S = 1, bool BNB = false>
__global__ void __launch_bounds__(256, BM == 64 ? 2 : 1) dconv_kernel(const DConvArgs a) {
    __shared__ float smem[dconv_lds_floats<OP, W, BM, CK, S, BNB>()];
    int bx, by, bz;
    block_xyz(bx, by, bz);
    dconv_body<OP, W, BM, WAVES_M, CK, WVEC, S, BNB>(a, smem, bx, by, bz);
}

// ---------------------------------------------------------------------------
// DGRAD of the 3x3 / stride-2 / pad-1 convolution (ResNet down-sampling blocks,
// models_pytorch.py:176-181) as a direct kernel.  dX pixel (2r+py, 2c+px) receives only
// the taps with 2r + py + 1 - kh even: kh = 1 for py = 0 (dY row r), kh in {0, 2} for
// py = 1 (rows r+1 and r), likewise kw / columns.  All four output parity phases therefore
// read ONE dY patch at the four shifts (dy, dx) in {0,1}^2:
//   dX[m][2r+py][2c+px] = sum_{ch, (kh,kw) of phase} W[ch][m][kh][kw] dY[ch][r+dy][c+dx]
// with py = (kh != 1), dy = (kh == 0) and the same for columns.  A workgroup owns 256
// dY-grid pixels (whole images: WG = 16 one image, WG = 8 four) x 32 dX channels, i.e.
// 1024 dX pixels; each wave keeps one 32x32 accumulator per (phase, 32-pixel tile) and
// issues, per channel pair, 18 MFMAs from 9 weight operands and 8 patch operands (all
// ds_read immediates).  The patch is staged per reduction channel as whole dY images plus
// a zero bottom row and right column (the +1 shifts past the map read zeros, written once).
// dX leaves as float2 (phases px = 0, 1 are adjacent).  Split over the reduction channels
// as dconv_kernel: the slab is laid out as the dX map itself (splitk_epilogue_kernel).
// (The implicit-GEMM phase path, igemm_kernel<OP_DGRAD_S2>, stays for 1x1 shortcuts and
// shapes this kernel does not take.)
// SC: the block's 1x1 / stride-2 projection shortcut (models_pytorch.py:183-187) reads the
// same input pixels (2r, 2c) = phase (0, 0), so its DGRAD joins that phase's accumulators: one
// more MFMA per channel pair from the shortcut's output gradient (staged per chunk as the
// tile's 256 grid pixels) and its 1x1 weights.  The separate launch, its mostly-zero dX write
// and this kernel's read-modify-write of dX disappear.
template <int WG, int CK, bool SC>
__global__ void __launch_bounds__(256, 2) dconv_dgrad_s2_kernel(const DConvArgs a) {
    constexpr int HG = WG, HWG = WG * WG;         // dY grid (= the conv's output map)
    constexpr int WX = 2 * WG, HWX = 4 * HWG;     // dX map
    constexpr int TR = 256 / WG, NI = TR / HG;    // grid rows / whole images per tile
    static_assert(TR % HG == 0 && NI >= 1 && WG % 4 == 0, "whole images per tile");
    constexpr int PRS = HG + 1, PW = WG + 1;      // patch rows per image (+ zero row), pitch
    constexpr int PR = NI * PRS;
    constexpr int CSTR = (PR * PW) | 1;           // odd: the two lane halves' channels
    constexpr int BM = 32, BMP = BM + 1;
    constexpr int KS = 9 * CK;
    constexpr int PE = CK * CSTR;
    constexpr int PQ = WG / 4, RPI = 256 / PQ, NPR = CK * NI * HG;
    constexpr int NPT = (NPR + RPI - 1) / RPI;
    constexpr int NAV = (BM * KS / 4 + 255) / 256;
    constexpr int FN = 2;                         // 64 grid pixels per wave
    static_assert((CK % 2) == 0, "channel pairs");
    // SC staging: the shortcut gradient [CK][256 (+1 pitch)], its weights [CK][BMP]
    constexpr int P2STR = 257, P2E = SC ? CK * P2STR : 0, A2E = SC ? CK * BMP : 0;
    constexpr int NQ2 = SC ? (CK * 64 + 255) / 256 : 0;    // float4 quads per thread
    constexpr int NA2 = SC ? (CK * BM + 255) / 256 : 0;    // weights per thread
    static_assert(!SC || (CK * 64) % 256 == 0, "shortcut staging");

    __shared__ float smem[2 * KS * BMP + 2 * PE + 2 * P2E + 2 * A2E];
    float (*As)[KS * BMP] = reinterpret_cast<float (*)[KS * BMP]>(smem);
    float (*Ps)[PE] = reinterpret_cast<float (*)[PE]>(smem + 2 * KS * BMP);
    float* P2s = smem + 2 * KS * BMP + 2 * PE;          // [2][P2E]
    float* A2s = P2s + 2 * P2E;                         // [2][A2E]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    int bx, by, bz;
    block_xyz(bx, by, bz);
    const int z = bz / a.splits;
    const int split = bz - z * a.splits;
    const int cnt = a.counts ? a.counts[z] : a.batch;
    const int t = bx, m0 = by * BM;
    const int n0 = t * 256;
    if (n0 >= cnt * HWG) return;
    const int cbeg = split * a.cchunk;
    const int cend = min(a.Cr, cbeg + a.cchunk);
    const int M = a.M;

    // zero halo of both buffers: each image's bottom row and every row's right column
    for (int q = tid; q < 2 * CK * PR; q += 256) {
        const int bsel = q / (CK * PR), row = q % (CK * PR);
        float* r = &Ps[bsel][(row / PR) * CSTR + (row % PR) * PW];
        if ((row % PR) % PRS == HG) {
#pragma unroll
            for (int x = 0; x < PW; ++x) r[x] = 0.f;
        } else {
            r[WG] = 0.f;
        }
    }

    const int img0 = t * NI;
    const int prt = tid / PQ, px4 = (tid % PQ) * 4;
    const float* inz = a.in + z * a.in_cs;
    const float* wz = a.wt + z * a.w_cs;
    float4 rp[NPT], ra[NAV];
    float4 rq[NQ2 > 0 ? NQ2 : 1];
    float rw[NA2 > 0 ? NA2 : 1];
    auto load = [&](int c0) {
        if constexpr (SC) {
            const float* in2z = a.in2 + z * a.in2_cs;
#pragma unroll
            for (int i = 0; i < NQ2; ++i) {  // quad f: channel f / 64, tile pixels 4 (f % 64) ..
                const int f = tid + i * 256, cl = f / 64, n = 4 * (f % 64);
                const int img = img0 + n / HWG;
                const bool ok = img < cnt && c0 + cl < cend;
                rq[i] = ok ? *reinterpret_cast<const float4*>(
                                 in2z + ((int64_t)img * a.Cr + c0 + cl) * HWG + n % HWG)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            const float* w2z = a.wt2 + z * a.w2_cs;
#pragma unroll
            for (int i = 0; i < NA2; ++i) {  // W_sc[c0 + cl][m0 + m] (layout [cout][cin])
                const int e = tid + i * 256, cl = e / BM, m = e % BM;
                rw[i] = (e < CK * BM && c0 + cl < cend && m0 + m < M)
                            ? w2z[(int64_t)(c0 + cl) * M + m0 + m] : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int q = prt + i * RPI;
            const int cl = q / (NI * HG), rem = q % (NI * HG);
            const int img = img0 + rem / HG, y = rem % HG;
            const bool ok = q < NPR && img < cnt && c0 + cl < cend;
            rp[i] = ok ? *reinterpret_cast<const float4*>(
                             inz + ((int64_t)(img * a.Cr + c0 + cl) * HG + y) * WG + px4)
                       : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < NAV; ++i) {  // run of 9*BM floats per ch: W[c0+cl][m0 .. m0+BM)[9]
            const int f = tid + i * 256;
            const int cl = f / (BM * 9 / 4), j4 = f % (BM * 9 / 4);
            ra[i] = (f < BM * KS / 4 && c0 + cl < cend)
                        ? *reinterpret_cast<const float4*>(wz + ((int64_t)(c0 + cl) * M + m0) * 9 +
                                                           4 * j4)
                        : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto store = [&](int buf) {
        if constexpr (SC) {
#pragma unroll
            for (int i = 0; i < NQ2; ++i) {
                const int f = tid + i * 256;
                float* d = P2s + buf * P2E + (f / 64) * P2STR + 4 * (f % 64);
                d[0] = rq[i].x;
                d[1] = rq[i].y;
                d[2] = rq[i].z;
                d[3] = rq[i].w;
            }
#pragma unroll
            for (int i = 0; i < NA2; ++i) {
                const int e = tid + i * 256;
                if (e < CK * BM) A2s[buf * A2E + (e / BM) * BMP + e % BM] = rw[i];
            }
        }
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int q = prt + i * RPI;
            if (q < NPR) {
                const int cl = q / (NI * HG), rem = q % (NI * HG);
                float* d = &Ps[buf][cl * CSTR + ((rem / HG) * PRS + rem % HG) * PW + px4];
                d[0] = rp[i].x;
                d[1] = rp[i].y;
                d[2] = rp[i].z;
                d[3] = rp[i].w;
            }
        }
#pragma unroll
        for (int i = 0; i < NAV; ++i) {
            const int f = tid + i * 256;
            if (f < BM * KS / 4) {
                const int cl = f / (BM * 9 / 4);
                const float vv[4] = {ra[i].x, ra[i].y, ra[i].z, ra[i].w};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = 4 * (f % (BM * 9 / 4)) + u, m = k / 9, r9 = k % 9;
                    As[buf][(r9 * CK + cl) * BMP + m] = (m0 + m < M) ? vv[u] : 0.f;
                }
            }
        }
    };

    f32x16 acc[4][FN];
#pragma unroll
    for (int ph = 0; ph < 4; ++ph)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ph][j][r] = 0.f;

    const int h = lane >> 5, col = lane & 31;
    const int a_lane = h * BMP + col;
    int b_lane[FN];
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int n = wid * 64 + j * 32 + col;  // local grid pixel
        const int il = n / HWG, p = n % HWG;
        b_lane[j] = h * CSTR + (il * PRS + p / WG) * PW + p % WG;
    }

    if (cbeg < cend) {
        load(cbeg);
        store(0);
        __syncthreads();
        int buf = 0;
        for (int c0 = cbeg; c0 < cend; c0 += CK) {
            const bool more = c0 + CK < cend;
            if (more) load(c0 + CK);
            const float* Ab = &As[buf][a_lane];
            const float* Pb = &Ps[buf][0];
            const float* A2b = A2s + buf * A2E + a_lane;
            const float* P2b = P2s + buf * P2E + h * P2STR + wid * 64 + col;
#pragma unroll
            for (int cp = 0; cp < CK / 2; ++cp) {
                float bv[4][FN], av[9];
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int j = 0; j < FN; ++j)
                        bv[s][j] = Pb[b_lane[j] + 2 * cp * CSTR + (s >> 1) * PW + (s & 1)];
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) av[tap] = Ab[(tap * CK + 2 * cp) * BMP];
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int kh = tap / 3, kw = tap % 3;
                    const int ph = (kh != 1) * 2 + (kw != 1), sh = (kh == 0) * 2 + (kw == 0);
#pragma unroll
                    for (int j = 0; j < FN; ++j)
                        acc[ph][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tap], bv[sh][j],
                                                                          acc[ph][j], 0, 0, 0);
                }
                if constexpr (SC) {  // the shortcut's 1x1: phase (0, 0), shift (0, 0)
                    const float a2 = A2b[2 * cp * BMP];
#pragma unroll
                    for (int j = 0; j < FN; ++j)
                        acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                            a2, P2b[2 * cp * P2STR + j * 32], acc[0][j], 0, 0, 0);
                }
            }
            if (more) store(buf ^ 1);
            __syncthreads();
            buf ^= 1;
        }
    }

    // ---- epilogue: per lane one grid pixel -> two float2 (px = 0, 1) per channel ----
    const int rbase = 4 * h;
    const bool split_out = a.splits > 1;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int n = n0 + wid * 64 + j * 32 + col;
        const int img = n / HWG, p = n % HWG, r = p / WG, c = p % WG;
        if (img >= cnt) continue;
#pragma unroll
        for (int py = 0; py < 2; ++py) {
            const int po = (2 * r + py) * WX + 2 * c;
            float* op = split_out ? a.out + ((int64_t)bz * M) * a.Nfull + (int64_t)img * HWX + po
                                  : a.out + z * a.out_cs + (int64_t)img * M * HWX + po;
            const int64_t ms = split_out ? (int64_t)a.Nfull : (int64_t)HWX;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int m = m0 + (rr & 3) + 8 * (rr >> 2) + rbase;
                if (m < M) {
                    float2 v = make_float2(acc[2 * py][j][rr], acc[2 * py + 1][j][rr]);
                    float2* q = reinterpret_cast<float2*>(op + (int64_t)m * ms);
                    if (!split_out && a.accumulate) {
                        const float2 o = *q;
                        v.x = o.x + v.x;
                        v.y = o.y + v.y;
                    }
                    *q = v;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// 1x1 / stride-2 / pad-0 FORWARD (the ResNet projection shortcut, models_pytorch.py:183-187):
// Y[m][r][c] = sum_ch W[m][ch] X[ch][2r][2c].  A workgroup owns 256 output pixels (whole
// images: WO = 16 one, WO = 8 four) x 64 output channels; per chunk of CK input channels it
// stages the even input rows as float4 runs keeping the even columns (x, z) — Xs[ch][256 +1]
// — and the weights as float4 runs of W[m][ch..] transposed into Ws[ch][64 +1]; 4 waves =
// 2 (channels) x 2 (pixel halves), 1 x 4 32x32 accumulators each.  The implicit GEMM
// gathered every operand with its own address arithmetic (2-4 % of peak); here the X read
// bounds it.
template <int WO, int CK>
__global__ void __launch_bounds__(256) pw_s2_fwd_kernel(const DConvArgs a) {
    constexpr int HWO = WO * WO, WI = 2 * WO, HI = 2 * WO;
    constexpr int NI = 256 / HWO;                 // whole output images per tile
    static_assert(256 % HWO == 0 && WO % 2 == 0, "tile geometry");
    constexpr int BM = 64, BMP = BM + 1, XP = 257;
    constexpr int QPC = 128;                      // float4 runs per channel (2 pixels each)
    constexpr int NQ = CK * QPC / 256, NW = CK * BM / 4 / 256;
    static_assert(NQ >= 1 && NW >= 1 && (CK * QPC) % 256 == 0 && (CK * BM / 4) % 256 == 0 &&
                  CK % 4 == 0, "staging");
    __shared__ float Xs[2][CK * XP];
    __shared__ float Ws[2][CK * BMP];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid >> 1, wn = wid & 1;
    const int z = blockIdx.z, t = blockIdx.x, m0 = blockIdx.y * BM;
    const int cnt = a.counts ? a.counts[z] : a.batch;
    const int n0 = t * 256;
    if (n0 >= cnt * HWO) return;
    const int M = a.M, Cr = a.Cr;
    const int img0 = t * NI;
    const float* xz = a.in + z * a.in_cs;
    const float* wz = a.wt + z * a.w_cs;

    float4 rx[NQ], rw[NW];
    auto load = [&](int c0) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int f = tid + i * 256, cl = f / QPC, n = 2 * (f % QPC);  // output pixels n, n+1
            const int il = n / HWO, p = n % HWO, r = p / WO, c = p % WO;
            const int img = img0 + il;
            rx[i] = (img < cnt && c0 + cl < Cr)
                        ? *reinterpret_cast<const float4*>(
                              xz + ((int64_t)(img * Cr + c0 + cl) * HI + 2 * r) * WI + 2 * c)
                        : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int f = tid + i * 256, m = f / (CK / 4), j4 = f % (CK / 4);
            rw[i] = (m0 + m < M && c0 + 4 * j4 < Cr)
                        ? *reinterpret_cast<const float4*>(wz + (int64_t)(m0 + m) * Cr + c0 + 4 * j4)
                        : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int f = tid + i * 256;
            float* d = &Xs[buf][(f / QPC) * XP + 2 * (f % QPC)];
            d[0] = rx[i].x;
            d[1] = rx[i].z;
        }
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int f = tid + i * 256, m = f / (CK / 4), j4 = f % (CK / 4);
            Ws[buf][(4 * j4 + 0) * BMP + m] = rw[i].x;
            Ws[buf][(4 * j4 + 1) * BMP + m] = rw[i].y;
            Ws[buf][(4 * j4 + 2) * BMP + m] = rw[i].z;
            Ws[buf][(4 * j4 + 3) * BMP + m] = rw[i].w;
        }
    };

    f32x16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    const int h = lane >> 5, col = lane & 31;
    load(0);
    store(0);
    __syncthreads();
    int buf = 0;
    for (int c0 = 0; c0 < Cr; c0 += CK) {
        const bool more = c0 + CK < Cr;
        if (more) load(c0 + CK);
        const float* Ab = &Ws[buf][h * BMP + wm * 32 + col];
        const float* Bb = &Xs[buf][h * XP + wn * 128 + col];
#pragma unroll
        for (int cp = 0; cp < CK / 2; ++cp) {
            const float av = Ab[2 * cp * BMP];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, Bb[2 * cp * XP + j * 32], acc[j],
                                                              0, 0, 0);
        }
        if (more) store(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }

    const float* bz = a.bias ? a.bias + z * a.b_cs : nullptr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + wn * 128 + j * 32 + col;
        const int img = n / HWO, p = n % HWO;
        if (img >= cnt) continue;
        float* op = a.out + z * a.out_cs + (int64_t)img * M * HWO + p;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (m < M) {
                float v = acc[j][r];
                if (bz) v = v + bz[m];
                if (a.relu) v = fmaxf(v, 0.f);
                op[(int64_t)m * HWO] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// WGRAD of the ResNet 3x3 / stride-2 / pad-1 down-sampling convolutions (r02; the stride-1
// layers moved to dwgrad_q_kernel below in r03):
// dW[co][ci][kh][kw] = sum_pix dY[co][pix] * X[ci][2 pix + (kh-1, kw-1)]
//
// The reduction runs over pixels, so MFMA lanes span co (A) and ci (B).  Each wave keeps
// nine 32x32 accumulators, one per (kh,kw) shift: per pixel pair it reads one dY operand
// and nine shifted patch operands (the shift is an LDS immediate) for nine MFMAs.  A stage
// is SR output rows of dY (staged [pix][co]) and the 2*SR+1 input rows they read with a zero
// halo (staged [ci][row][2W+2], channel stride odd so 32 channels on 32 lanes hit 32 banks).
// The four waves tile (co, ci, pixel-rows); waves that split pixels are summed through LDS
// in a fixed order.  Every workgroup writes its partial for one pixel split into the slab
// [z][split][co][ci*9+s] (the conv bias gradient = sum of dY rows rides along), reduced by
// splitk_sum_kernel.
struct DWArgs {
    const float* x;
    const float* dy;
    float* part;       // [z][split][M][N]
    float* bias_part;  // [z][split][M] or null
    int64_t x_cs, dy_cs;
    const int32_t* counts;
    int batch, cin, M, N;  // M = cout, N = cin*9
    int splits, stages_per_split;
    // nullable: x is a BatchNorm pre-activation, staged as relu(x * scale + shift)
    const float* in_scale;
    const float* in_shift;
    int64_t aff_cs;
    // dwgrad_q_kernel with splits == 1: dW (and db when non-null) written directly
    float* dw;
    int64_t dw_cs;
    float* db;
    int64_t db_cs;
    // dwgrad_q (the dual-role launch's WGRAD role), PDY: dY routed from a 2x2 max-pool's gradient
    PooledDy pdy;
};

// Two workgroups per CU when the double-buffered staging fits twice in the 160 KB LDS:
// then ask the allocator for two waves per SIMD (host planner: the same formula, conv.hip
// plan_dwgrad_s2).  W = the OUTPUT width: a stage's patch is the 2*SEGR+1 input rows its
// output rows read, 2W+2 wide with the halo, and a lane's operand address strides by 2.
constexpr int dwgrad_occ(int W, int WCO, int WCI, int SR, int S = 1) {
    const int SEGR = SR < W ? SR : W, NI = SR / SEGR;
    const int PR = NI * (S == 1 ? SEGR + 2 : 2 * SEGR + 1), CSTR = (PR * (S * W + 2)) | 1;
    const int bytes = 4 * (2 * SR * W * (32 * WCO + 1) + 2 * 32 * WCI * CSTR);
    return 2 * bytes <= 160 * 1024 ? 2 : 1;
}

template <int W, int WCO, int WCI, int WPX, int SR, int S>
__global__ void __launch_bounds__(256, dwgrad_occ(W, WCO, WCI, SR, S)) dconv_wgrad_kernel(const DWArgs a) {
    constexpr int H = W, HW = H * W;                // output map
    constexpr int WI = S * W, HI = S * H;           // input map
    constexpr int SPX = SR * W;                     // pixels per stage
    constexpr int SEGR = SR < H ? SR : H;
    constexpr int NI = SR / SEGR;
    constexpr int PRS = S == 1 ? SEGR + 2 : 2 * SEGR + 1;  // patch rows per image segment
    constexpr int PW = WI + 2, PR = NI * PRS;
    constexpr int CSTR = (PR * PW) | 1;
    constexpr int BM = 32 * WCO, BN = 32 * WCI;
    constexpr int BMP = BM + 1;
    constexpr int RPW = SR / WPX;                   // rows per wave per stage
    // staging with float4 global loads: dY rows of SPX pixels, patch rows of W pixels
    constexpr int DQ = SPX / 4, COI = 256 / DQ, NDY = BM / COI;
    constexpr int PQ = WI / 4, RPI = 256 / PQ, NPR = BN * PR, NPT = (NPR + RPI - 1) / RPI;
    constexpr int DSZ = SPX * BMP, PSZ = BN * CSTR, BUF = DSZ + PSZ;
    static_assert(WCO * WCI * WPX == 4 && RPW >= 1 && SR % WPX == 0, "wave grid");
    static_assert(S == 1 || S == 2, "stride");
    static_assert(BM % COI == 0 && (SR % H == 0 || H % SR == 0), "stage geometry");

    constexpr int SMEM = 2 * BUF;
    __shared__ float smem[SMEM];   // double-buffered [Dys | Ps]
    auto dbase = [](int bsel) { return bsel * BUF; };
    auto pbase = [](int bsel) { return bsel * BUF + DSZ; };

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wpx = wid % WPX, wci = (wid / WPX) % WCI, wco = wid / (WPX * WCI);
    int bx, by, bz;
    block_xyz(bx, by, bz);
    const int split = bx, z = bz;
    const int ntile_ci = a.cin / BN;
    const int co0 = (by / ntile_ci) * BM, ci0 = (by % ntile_ci) * BN;
    const int cnt = a.counts ? a.counts[z] : a.batch;
    const int nst = (cnt * HW + SPX - 1) / SPX;
    const int sbeg = split * a.stages_per_split;
    const int send = min(nst, sbeg + a.stages_per_split);
    const float* xz = a.x + z * a.x_cs;
    const float* dyz = a.dy + z * a.dy_cs;
    const bool do_bias = a.bias_part != nullptr && ci0 == 0;

    // halo columns of the patch are always zero (pad = 1): write them once
    for (int q = tid; q < 2 * NPR; q += 256) {
        const int bsel = q / NPR, row = q % NPR, cl = row / PR, pr = row % PR;
        float* r = smem + pbase(bsel) + cl * CSTR + pr * PW;
        r[0] = 0.f;
        r[WI + 1] = 0.f;
    }

    const int dco = tid / DQ, dp = (tid % DQ) * 4;      // dY: channel row, pixel quad
    const int prt = tid / PQ, px = (tid % PQ) * 4;       // patch: row, column quad
    float4 rd[NDY], rp[NPT];
    float bsc[NPT], bsh[NPT];  // BN affine of each staged X row (in_scale set)
    auto load = [&](int st) {
        const int R0 = st * SR;
        {
            const int row = R0 + dp / W, img = row / H, y = row % H, xx = dp % W;
            const float* src = dyz + ((int64_t)(img * a.M + co0 + dco) * H + y) * W + xx;
            const bool ok = img < cnt;
#pragma unroll
            for (int i = 0; i < NDY; ++i)
                rd[i] = ok ? *reinterpret_cast<const float4*>(src + (int64_t)i * COI * HW)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const int img0 = R0 / H, y0 = R0 % H;
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int q = prt + i * RPI;
            const int cl = q / PR, pr = q % PR;
            const int seg = pr / PRS, rr = pr % PRS;
            const int img = img0 + seg, y = S * y0 + rr - 1;
            const bool ok = q < NPR && img < cnt && (unsigned)y < (unsigned)HI;
            rp[i] = ok ? *reinterpret_cast<const float4*>(
                             xz + ((int64_t)(img * a.cin + ci0 + cl) * HI + y) * WI + px)
                       : make_float4(0.f, 0.f, 0.f, 0.f);
            if (a.in_scale != nullptr) {  // applied in store() (loads stay in flight)
                bsc[i] = ok ? a.in_scale[z * a.aff_cs + ci0 + cl] : 1.f;
                bsh[i] = ok ? a.in_shift[z * a.aff_cs + ci0 + cl] : 0.f;
            }
        }
    };
    auto store_d = [&](int bsel) {
        float* D = smem + dbase(bsel);
#pragma unroll
        for (int i = 0; i < NDY; ++i) {
            float* d = D + dp * BMP + dco + i * COI;
            d[0] = rd[i].x;
            d[BMP] = rd[i].y;
            d[2 * BMP] = rd[i].z;
            d[3 * BMP] = rd[i].w;
        }
    };
    auto store_p = [&](int bsel) {
        float* P = smem + pbase(bsel);
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int q = prt + i * RPI;
            if (q < NPR) {
                if (a.in_scale != nullptr) rp[i] = bn_relu4(rp[i], bsc[i], bsh[i]);
                float* d = P + (q / PR) * CSTR + (q % PR) * PW + 1 + px;
                d[0] = rp[i].x;
                d[1] = rp[i].y;
                d[2] = rp[i].z;
                d[3] = rp[i].w;
            }
        }
    };
    auto store = [&](int bsel) {
        store_d(bsel);
        store_p(bsel);
    };

    f32x16 acc[9];
#pragma unroll
    for (int s = 0; s < 9; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
    float bsum = 0.f;

    const int h = lane >> 5, col = lane & 31;
    const int a_off = h * BMP + wco * 32 + col;
    const int b_off = (wci * 32 + col) * CSTR + S * h;
    if (sbeg < send) {
        load(sbeg);
        store(0);
        __syncthreads();
        int bsel = 0;
        for (int st = sbeg; st < send; ++st) {
            const bool more = st + 1 < send;
            if (more) load(st + 1);
            const float* Al = smem + dbase(bsel) + a_off;
            const float* Bl = smem + pbase(bsel) + b_off;
#pragma unroll 1
            for (int rr = 0; rr < RPW; ++rr) {
                const int r = wpx * RPW + rr;                  // stage row
                const int prow = (r / SEGR) * PRS + S * (r % SEGR);
                const float* Ar = Al + r * W * BMP;
                const float* Br = Bl + prow * PW;
#pragma unroll 4
                for (int cp = 0; cp < W / 2; ++cp) {
                    const float av = Ar[2 * cp * BMP];
                    bsum += av;
                    float bv[9];
#pragma unroll
                    for (int s = 0; s < 9; ++s) bv[s] = Br[(s / 3) * PW + S * 2 * cp + (s % 3)];
#pragma unroll
                    for (int s = 0; s < 9; ++s)
                        acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[s], acc[s], 0, 0, 0);
                }
            }
            if (more) store(bsel ^ 1);
            __syncthreads();
            bsel ^= 1;
        }
    }

    // ---- combine the WPX pixel waves (fixed order), then write the slab --
    __syncthreads();    // halo / staging writes retired before the scratch is reused
    float* red = smem;  // staging LDS reused as reduction scratch
    const int64_t slab = ((int64_t)z * a.splits + split) * a.M;
    constexpr int WT = WCO * WCI;
    if constexpr (WPX > 1) {
        // every wave parks 3 shifts of its accumulators in LDS; then all 256 threads sum
        // the WPX pixel partials (fixed order) and write the slab
        constexpr int SG = (WPX * WT * 3 * 16 * 64 <= SMEM) ? 3 : 1;  // shifts per round
        static_assert(WPX * WT * SG * 16 * 64 <= SMEM, "reduction scratch");
        const int wt_me = wco * WCI + wci;
        float* op = a.part + slab * a.N;
#pragma unroll
        for (int g = 0; g < 9; g += SG) {
#pragma unroll
            for (int s = 0; s < SG; ++s)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    red[(((wpx * WT + wt_me) * SG + s) * 16 + r) * 64 + lane] = acc[g + s][r];
            __syncthreads();
#pragma unroll 1
            for (int e = tid; e < WT * SG * 1024; e += 256) {
                const int wt = e / (SG * 1024), rem = e % (SG * 1024);
                const int sh = rem / 1024, r = (rem / 64) % 16, l = rem % 64;
                float v = 0.f;
#pragma unroll
                for (int q = 0; q < WPX; ++q) v += red[((q * WT + wt) * SG * 1024) + rem];
                const int m = co0 + (wt / WCI) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
                const int ci = ci0 + (wt % WCI) * 32 + (l & 31);
                op[(int64_t)m * a.N + ci * 9 + g + sh] = v;
            }
            __syncthreads();
        }
    }
    // bias: lanes l and l+32 hold different pixels of the same co
    if (do_bias) {  // block-uniform: every wave reaches the barrier
        float* bred = red;
        if (wci == 0) bred[wid * 64 + lane] = bsum;
        __syncthreads();
        if (wci == 0 && wpx == 0 && lane < 32) {
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < WPX; ++q) {
                const int w2 = wco * WCI * WPX + q;  // wci == 0
                v += bred[w2 * 64 + lane] + bred[w2 * 64 + lane + 32];
            }
            a.bias_part[slab + co0 + wco * 32 + lane] = v;
        }
    }
    if (WPX == 1) {
        float* op = a.part + slab * a.N;
        const int ci = ci0 + wci * 32 + col;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = co0 + wco * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
#pragma unroll
            for (int s = 0; s < 9; ++s) op[(int64_t)m * a.N + ci * 9 + s] = acc[s][r];
        }
    }
}

// ---------------------------------------------------------------------------
// WGRAD, 3x3 / stride 1 / pad 1 (r03): dW[co][ci][kh][kw] = sum_pix dY[co][pix] X[ci][pix+s].
//
// A workgroup owns a 32x32 (co, ci) tile of one client and a run of SPX-pixel stages; each
// of its four waves owns one 16x16 quadrant of the tile for all nine shifts (nine
// v_mfma_f32_16x16x4_f32 accumulators, 36 registers) and walks EVERY pixel of the stage, four
// pixels (the MFMA's k) at a time: one dY operand and nine shifted patch operands (the shift
// is an LDS immediate) per nine MFMAs.  Against the r01/r02 kernel (32x32x2 MFMAs, 144
// accumulator registers per wave, pixels split over the four waves) this
//   * drops the cross-wave LDS combine of the epilogue — a wave's sums are final for its
//     split, the tile goes out through one LDS transpose as coalesced rows;
//   * fits three workgroups in a CU (<= 53 KB of LDS, <= 168 registers): dY [32 co][SPX+2]
//     and the patch [32 ci][rows][W+4], both pitches = 2 (mod 4) so a 16-lane x 2-k operand
//     read touches 32 distinct banks;
//   * keeps the summation order a pure function of the plan (per split: stages in order,
//     pixels in order inside a stage; splits summed in order by splitk_sum_kernel).
// DB = false: one 128-pixel staging buffer; the next stage's global loads go to registers
// while this stage is multiplied and are written to LDS between two barriers.
// DB = true: two 64-pixel buffers; the next stage is written to the other buffer half-way
// through this stage's MFMAs, one barrier per stage (the workgroups on a CU start together,
// so with one buffer their store phases coincide and nothing hides them).
// splits == 1 (many tiles): dW / db written directly, no reduction launch.
constexpr int dwq_buf_floats(int W, int SPX) {
    const int SR = SPX / W, SEGR = SR < W ? SR : W, NI = SR / SEGR;
    return 32 * (SPX + 2) + 32 * (NI * (SEGR + 2) * (W + 4) + 2);
}
constexpr int dwq_lds_floats(int W, int SPX, bool DB) {
    const int st = (DB ? 2 : 1) * dwq_buf_floats(W, SPX);
    return st > 32 * 289 + 128 ? st : 32 * 289 + 128;
}

template <int W, int SPX, bool DB, bool PDY = false>
__device__ __forceinline__ void dwgrad_q_body(const DWArgs& a, float* smem, int bx, int by,
                                              int bz) {
    constexpr int H = W, HW = H * W;
    constexpr int SR = SPX / W;
    constexpr int SEGR = SR < H ? SR : H, NI = SR / SEGR;
    constexpr int PRS = SEGR + 2, PW = W + 4, PR = NI * PRS;
    constexpr int CSTR = PR * PW + 2;  // = 2 (mod 4): lanes (m, k) -> banks 2m*odd + k, distinct
    constexpr int DP = SPX + 2;        // dY pitch, = 2 (mod 4) likewise
    constexpr int DSZ = 32 * DP, BUF = dwq_buf_floats(W, SPX);
    constexpr int DQ = SPX / 4, CPP = 256 / DQ, NDY = 32 / CPP;  // dY float4s per thread
    constexpr int PQ = W / 4, NPQ = 32 * PR * PQ;               // patch float4s
    constexpr int NPT = (NPQ + 255) / 256;                       // ... per thread
    constexpr int RP = 289;                                      // epilogue row pitch
    static_assert(256 % DQ == 0 && 32 % CPP == 0, "staging");
    static_assert(SR % SEGR == 0 && (SR <= H || SR % H == 0), "stage geometry");
    static_assert(!DB || SR % 2 == 0 || SR == 1, "half-stage store point");
    static_assert(dwq_lds_floats(W, SPX, DB) * 4 <= 160 * 1024 / 3, "three workgroups per CU");

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cq = wid & 1, nq = wid >> 1;  // this wave's 16x16 quadrant (co half, ci half)
    const int split = bx, z = bz;
    const int ntile_ci = a.cin / 32;
    const int co0 = (by / ntile_ci) * 32, ci0 = (by % ntile_ci) * 32;
    const int cnt = a.counts ? a.counts[z] : a.batch;
    const int nst = (cnt * HW + SPX - 1) / SPX;
    const int sbeg = split * a.stages_per_split;
    const int send = min(nst, sbeg + a.stages_per_split);
    const float* xz = a.x + z * a.x_cs;
    const float* dyz = a.dy + z * a.dy_cs;
    const bool do_bias = (a.bias_part != nullptr || a.db != nullptr) && ci0 == 0;

    // zero halo columns (image columns -1 and W): written once, never overwritten
    for (int q = tid; q < (DB ? 2 : 1) * 32 * PR; q += 256) {
        const int b = q / (32 * PR), r0 = q % (32 * PR);
        float* r = smem + b * BUF + DSZ + (r0 / PR) * CSTR + (r0 % PR) * PW;
        r[1] = 0.f;
        r[W + 2] = 0.f;
    }

    const int dq = tid % DQ, dco = tid / DQ;  // dY: pixel quad, first channel row
    float4 rd[NDY], rp[NPT];
    float bsc[NPT], bsh[NPT];
    float2 pg[PDY ? NDY : 1], pp[PDY ? NDY : 1];  // PDY: raw pooled loads, routed in store()
    int pc[PDY ? NDY : 1];
    auto load = [&](int st) {
        const int gp = st * SPX + 4 * dq;
        const int img = gp / HW, pix = gp % HW;
        const bool ok = img < cnt;
        const float* src = dyz + ((int64_t)(img * a.M + co0 + dco) * HW + pix);
#pragma unroll
        for (int i = 0; i < NDY; ++i) {
            if constexpr (PDY) {
                pdy_load(a.pdy, z, (int64_t)img * a.M + co0 + dco + i * CPP, pix / W, pix % W, ok,
                         pg[i], pp[i], pc[i]);
                continue;
            }
            rd[i] = ok ? *reinterpret_cast<const float4*>(src + (int64_t)i * CPP * HW)
                       : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const int img0 = (st * SPX) / HW, y0 = ((st * SPX) % HW) / W;
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int q = tid + 256 * i;
            const int quad = q % PQ, row = q / PQ, ci = row / PR, pr = row % PR;
            const int im = img0 + pr / PRS, y = y0 + pr % PRS - 1;
            const bool okp = (NPQ % 256 == 0 || q < NPQ) && im < cnt && (unsigned)y < (unsigned)H;
            rp[i] = okp ? *reinterpret_cast<const float4*>(
                              xz + ((int64_t)(im * a.cin + ci0 + ci) * HW + y * W + 4 * quad))
                        : make_float4(0.f, 0.f, 0.f, 0.f);
            if (a.in_scale != nullptr) {  // applied in store(): the loads stay in flight
                bsc[i] = okp ? a.in_scale[z * a.aff_cs + ci0 + ci] : 1.f;
                bsh[i] = okp ? a.in_shift[z * a.aff_cs + ci0 + ci] : 0.f;
            }
        }
    };
    auto store = [&](int b) {
        float* D = smem + b * BUF;
        float* P = D + DSZ;
#pragma unroll
        for (int i = 0; i < NDY; ++i) {
            if constexpr (PDY) rd[i] = pdy_route(pg[i], pp[i], pc[i]);
            float2* d = reinterpret_cast<float2*>(D + (dco + i * CPP) * DP + 4 * dq);
            d[0] = make_float2(rd[i].x, rd[i].y);
            d[1] = make_float2(rd[i].z, rd[i].w);
        }
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int q = tid + 256 * i;
            if (NPQ % 256 != 0 && q >= NPQ) continue;
            const int quad = q % PQ, row = q / PQ, ci = row / PR, pr = row % PR;
            if (a.in_scale != nullptr) rp[i] = bn_relu4(rp[i], bsc[i], bsh[i]);
            float2* d = reinterpret_cast<float2*>(P + ci * CSTR + pr * PW + 2 + 4 * quad);
            d[0] = make_float2(rp[i].x, rp[i].y);
            d[1] = make_float2(rp[i].z, rp[i].w);
        }
    };

    f32x4 acc[9];
#pragma unroll
    for (int s = 0; s < 9; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    const int m = lane & 15, kk = lane >> 4;
    const int a_off = (cq * 16 + m) * DP + kk;
    const int b_off = DSZ + (nq * 16 + m) * CSTR + kk + 1;
    const bool bias_wave = do_bias && nq == 0;
    auto rows = [&](int b, int r0, int r1) {
        const float* Ab = smem + b * BUF + a_off;
        const float* Bb = smem + b * BUF + b_off;
#pragma unroll 1
        for (int r = r0; r < r1; ++r) {
            const float* Ar = Ab + r * W;
            const float* Br = Bb + ((r / SEGR) * PRS + r % SEGR) * PW;
#pragma unroll
            for (int g = 0; g < W / 4; ++g) {
                const float av = Ar[4 * g];
                float bv[9];
#pragma unroll
                for (int s = 0; s < 9; ++s) bv[s] = Br[(s / 3) * PW + 4 * g + (s % 3)];
                if (bias_wave) bsum += av;
#pragma unroll
                for (int s = 0; s < 9; ++s)
                    acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[s], acc[s], 0, 0, 0);
            }
        }
    };

    if (sbeg < send) {
        load(sbeg);
        store(0);
        __syncthreads();
        int b = 0;
        for (int st = sbeg; st < send; ++st) {
            const bool more = st + 1 < send;
            if (more) load(st + 1);
            if constexpr (DB) {
                constexpr int HALF = SR / 2 > 0 ? SR / 2 : 1;
                rows(b, 0, HALF);
                if (more) store(b ^ 1);  // the other buffer: last read before the barrier
                rows(b, HALF, SR);
                __syncthreads();
                b ^= 1;
            } else {
                if constexpr (PDY && SR <= H) {
                    // rows past the pooled map's 2 ph rows carry a zero gradient: skipping them
                    // adds nothing the MFMA chain would not have added as exact zeros
                    const int y0 = ((st * SPX) % HW) / W;
                    rows(0, 0, max(0, min(SR, 2 * a.pdy.ph - y0)));
                } else {
                    rows(0, 0, SR);
                }
                if (more) {
                    __syncthreads();  // every wave is done reading this stage
                    store(0);
                    __syncthreads();
                }
            }
        }
    }

    // ---- epilogue: the tile through LDS as [co][ci*9 + s] rows, then coalesced stores ----
    __syncthreads();
    float* red = smem;
#pragma unroll
    for (int s = 0; s < 9; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            red[(cq * 16 + 4 * kk + j) * RP + (nq * 16 + m) * 9 + s] = acc[s][j];
    float* bred = smem + 32 * RP;
    if (bias_wave) bred[cq * 64 + lane] = bsum;
    __syncthreads();
    const bool direct = a.splits == 1 && a.dw != nullptr;
    const int64_t slab = ((int64_t)z * a.splits + split) * a.M;
    float* out = direct ? a.dw + z * a.dw_cs : a.part + slab * a.N;
#pragma unroll 4
    for (int e = tid; e < 32 * 288; e += 256) {
        const int co = e / 288, n = e - co * 288;
        out[(int64_t)(co0 + co) * a.N + ci0 * 9 + n] = red[co * RP + n];
    }
    if (do_bias && tid < 32) {  // lanes l, l+16, l+32, l+48 of a wave: the same co
        const float* bb = bred + (tid >> 4) * 64 + (tid & 15);
        const float v = ((bb[0] + bb[16]) + bb[32]) + bb[48];
        if (direct) {
            if (a.db != nullptr) a.db[z * a.db_cs + co0 + tid] = v;
        } else {
            a.bias_part[slab + co0 + tid] = v;
        }
    }
}

template <int W, int SPX, bool DB>
__global__ void __launch_bounds__(256, 3) dwgrad_q_kernel(const DWArgs a) {
    __shared__ float smem[dwq_lds_floats(W, SPX, DB)];
    int bx, by, bz;
    block_xyz(bx, by, bz);
    dwgrad_q_body<W, SPX, DB>(a, smem, bx, by, bz);
}

// Launch timestamps (r05, fh_launch_ts_set): bench.py's roofline is the dual launch's average
// begin-to-end duration over the TIMED rounds, the quantity a kernel trace reports.  HIP events
// around the launches of concurrent lanes perturbed the rounds (K2 -8 %) and timed the queue
// waits as well; here each workgroup of a selected layer shape reads the 100 MHz wall clock
// at entry and, after a barrier, at exit, and appends {dispatch packet, shape, t0, t1} with one
// vector atomic and one 16-B store — the host groups the records per dispatch.
struct LaunchTs {
    uint32_t* rec;    // [cap][4]
    uint32_t* count;  // next free record (caller-zeroed)
    uint32_t cap;
    uint32_t shape;   // dual_shape_key of the layer recorded (0: none)
};
__device__ LaunchTs g_launch_ts;
__host__ __device__ constexpr uint32_t dual_shape_key(int w, int cin, int cout) {
    return (uint32_t)w | ((uint32_t)cin << 8) | ((uint32_t)cout << 20);
}

// A layer's WGRAD (dwgrad_q, 128-pixel stages) and DGRAD (dconv, BM = 32, CK = 8) read the
// same output gradient and write disjoint outputs: one launch runs both, the nw workgroups
// of the WGRAD grid (wx, wy, z) first (wfirst) or after the nd of the DGRAD grid (dx, dy, z),
// each x-fastest as in its own launch.  The layer's backward is then one dependent step instead of
// two, and the two grids fill each other's tails.
template <int W, bool BNB, bool PDY = false>
__global__ void __launch_bounds__(256, 3)
    dconv_wgrad_dual_kernel(const DWArgs wa, int wx, int wy, int nw, const DConvArgs da, int dx,
                            int dy, int nd, int wfirst) {
    constexpr int LW = dwq_lds_floats(W, 128, false);
    constexpr int LD = dconv_lds_floats<OP_DGRAD, W, 32, 8, 1, BNB>();
    __shared__ float smem[LW > LD ? LW : LD];
    const int b = blockIdx.x;
    const bool isw = wfirst ? b < nw : b >= nd;
    // launch timestamps: block-uniform (the DGRAD args carry the layer: M = cin, Cr = cout)
    const LaunchTs ts = g_launch_ts;
    const bool stamp = ts.rec != nullptr && ts.shape == dual_shape_key(W, da.M, da.Cr);
    const uint64_t t0 = stamp ? wall_clock64() : 0;
    if (isw) {
        const int q = wfirst ? b : b - nd;
        const int bz = q / (wx * wy), r = q - bz * wx * wy;
        dwgrad_q_body<W, 128, false, PDY>(wa, smem, r % wx, r / wx, bz);
    } else {
        const int q = wfirst ? b - nw : b;
        const int bz = q / (dx * dy), r = q - bz * dx * dy;
        dconv_body<OP_DGRAD, W, 32, 1, 8, true, 1, BNB, PDY>(da, smem, r % dx, r / dx, bz);
    }
    if (stamp) {
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint64_t t1 = wall_clock64();
            const uint32_t i = atomicAdd(ts.count, 1u);
            if (i < ts.cap) {
                const uint32_t key =
                    (uint32_t)(reinterpret_cast<uintptr_t>(__builtin_amdgcn_dispatch_ptr()) >> 6);
                *reinterpret_cast<uint4*>(ts.rec + 4 * (size_t)i) =
                    make_uint4(key, ts.shape, (uint32_t)t0, (uint32_t)t1);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// WGRAD for a small input-channel count (CIN*9 <= 32, e.g. the RGB first layer): the
// MFMA B lanes span the whole (ci,kh,kw) axis at once (lane l -> its own patch offset,
// lanes >= CIN*9 read a zero), one 32x32 accumulator per wave, four waves splitting
// the pixels of a stage; same staging, slab and bias folding as dconv_wgrad_kernel.
template <int W, int CIN>
__global__ void __launch_bounds__(256) dconv_wgrad_small_kernel(const DWArgs a) {
    constexpr int H = W, HW = H * W;
    constexpr int SR = 128 / W, SPX = SR * W;
    constexpr int SEGR = SR < H ? SR : H;
    constexpr int NI = SR / SEGR;
    constexpr int PW = W + 2, PR = NI * (SEGR + 2);
    constexpr int CSTR = PR * PW;
    constexpr int BMP = 33;
    constexpr int RPW = SR / 4;
    constexpr int DQ = SPX / 4, COI = 256 / DQ, NDY = 32 / COI;
    constexpr int PQ = W / 4, RPI = 256 / PQ, NPR = CIN * PR, NPT = (NPR + RPI - 1) / RPI;
    constexpr int DSZ = SPX * BMP, PSZ = CIN * CSTR;
    constexpr int BUF = DSZ + PSZ;
    static_assert(CIN * 9 <= 32 && SR % 4 == 0 && (SR % H == 0 || H % SR == 0), "geometry");

    __shared__ float smem[2 * BUF];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wpx = __builtin_amdgcn_readfirstlane(tid >> 6);
    int bx, by, bz;
    block_xyz(bx, by, bz);
    const int split = bx, z = bz;
    const int co0 = by * 32;
    const int cnt = a.counts ? a.counts[z] : a.batch;
    const int nst = (cnt * HW + SPX - 1) / SPX;
    const int sbeg = split * a.stages_per_split;
    const int send = min(nst, sbeg + a.stages_per_split);
    const float* xz = a.x + z * a.x_cs;
    const float* dyz = a.dy + z * a.dy_cs;

    for (int q = tid; q < 2 * NPR; q += 256) {
        const int bsel = q / NPR, row = q % NPR;
        float* r = smem + bsel * BUF + DSZ + (row / PR) * CSTR + (row % PR) * PW;
        r[0] = 0.f;
        r[W + 1] = 0.f;
    }

    const int dco = tid / DQ, dp = (tid % DQ) * 4;
    const int prt = tid / PQ, px = (tid % PQ) * 4;
    float4 rd[NDY], rp[NPT];
    auto load = [&](int st) {
        const int R0 = st * SR;
        {
            const int row = R0 + dp / W, img = row / H, y = row % H, xx = dp % W;
            const float* src = dyz + ((int64_t)(img * a.M + co0 + dco) * H + y) * W + xx;
            const bool ok = img < cnt;
#pragma unroll
            for (int i = 0; i < NDY; ++i)
                rd[i] = ok ? *reinterpret_cast<const float4*>(src + (int64_t)i * COI * HW)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const int img0 = R0 / H, y0 = R0 % H;
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int q = prt + i * RPI;
            const int cl = q / PR, pr = q % PR;
            const int seg = pr / (SEGR + 2), rr = pr % (SEGR + 2);
            const int img = img0 + seg, y = y0 + rr - 1;
            const bool ok = q < NPR && img < cnt && (unsigned)y < (unsigned)H;
            rp[i] = ok ? *reinterpret_cast<const float4*>(
                             xz + ((int64_t)(img * CIN + cl) * H + y) * W + px)
                       : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto store = [&](int bsel) {
        float* D = smem + bsel * BUF;
#pragma unroll
        for (int i = 0; i < NDY; ++i) {
            float* d = D + dp * BMP + dco + i * COI;
            d[0] = rd[i].x;
            d[BMP] = rd[i].y;
            d[2 * BMP] = rd[i].z;
            d[3 * BMP] = rd[i].w;
        }
        float* P = D + DSZ;
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int q = prt + i * RPI;
            if (q < NPR) {
                float* d = P + (q / PR) * CSTR + (q % PR) * PW + 1 + px;
                d[0] = rp[i].x;
                d[1] = rp[i].y;
                d[2] = rp[i].z;
                d[3] = rp[i].w;
            }
        }
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float bsum = 0.f;
    const int h = lane >> 5, col = lane & 31;
    // lane's (ci,kh,kw); lanes >= CIN*9 alias lane 0 (their output columns are dropped)
    const int nl = col < CIN * 9 ? col : 0;
    const int ci = nl / 9, kh = (nl % 9) / 3, kw = nl % 3;
    const int a_off = h * BMP + col;
    if (sbeg < send) {
        load(sbeg);
        store(0);
        __syncthreads();
        int bsel = 0;
        for (int st = sbeg; st < send; ++st) {
            const bool more = st + 1 < send;
            if (more) load(st + 1);
            const float* Al = smem + bsel * BUF + a_off;
            const float* P = smem + bsel * BUF + DSZ;
#pragma unroll 1
            for (int rr = 0; rr < RPW; ++rr) {
                const int r = wpx * RPW + rr;
                const int prow = (r / SEGR) * (SEGR + 2) + r % SEGR;
                const float* Ar = Al + r * W * BMP;
                const float* Br = P + ci * CSTR + (prow + kh) * PW + kw + h;
#pragma unroll 8
                for (int cp = 0; cp < W / 2; ++cp) {
                    const float av = Ar[2 * cp * BMP];
                    bsum += av;
                    const float bv = Br[2 * cp];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
                }
            }
            if (more) store(bsel ^ 1);
            __syncthreads();
            bsel ^= 1;
        }
    }
    __syncthreads();
    float* red = smem;
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(wpx * 16 + r) * 64 + lane] = acc[r];
    red[4 * 16 * 64 + wpx * 64 + lane] = bsum;
    __syncthreads();
    const int64_t slab = ((int64_t)z * a.splits + split) * a.M;
    float* op = a.part + slab * a.N;
    for (int e = tid; e < 16 * 64; e += 256) {
        const int r = e / 64, l = e % 64;
        const float v = ((red[(0 * 16 + r) * 64 + l] + red[(1 * 16 + r) * 64 + l]) +
                         red[(2 * 16 + r) * 64 + l]) + red[(3 * 16 + r) * 64 + l];
        const int m = co0 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
        const int n = l & 31;
        if (n < CIN * 9) op[(int64_t)m * a.N + n] = v;
    }
    if (a.bias_part && tid < 32) {
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            v += red[4 * 16 * 64 + q * 64 + tid] + red[4 * 16 * 64 + q * 64 + tid + 32];
        a.bias_part[slab + co0 + tid] = v;
    }
}

}  // namespace fh
