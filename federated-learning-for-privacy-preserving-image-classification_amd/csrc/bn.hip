// bn.hip — BatchNorm2d for client-packed activations (train fwd / eval fwd / bwd).
//
// Reference: nn.BatchNorm2d in CIFAR10CNN and FederatedResNet
// (src/shared/models_pytorch.py:108-120, 176-187), train-mode statistics over
// the valid images of each client, momentum 0.1, eps 1e-5, unbiased running
// variance — ATen CPU accumulates these in double (acc_type<float>); so do we.
//
// Each (client, channel) reduction is split over S blocks ("slices" of the
// channel's cnt*HW elements) so that even one client fills the chip; the S
// partials go to a caller workspace and are merged in a fixed order by the
// second kernel (deterministic).  Element loops are float4 when HW % 4 == 0.
//   train fwd : stats  (read x)            -> partial (sum x, sum x^2) in fp64
//               apply  (read x [,res], write y = relu?(x*alpha + beta [+res]))
//   bwd       : reduce (read dy, y, x [, write dres])  -> partial (sum g, sum (x-mean) g)
//               apply  (read dy, y, x, write dx = ((g - mean g) - (x-mean) k) invstd w)
// Fused: the ReLU that follows BN (forward) and its mask (backward, g = dy*(y>0)),
// and the ResNet residual add (forward) / residual-branch gradient (backward).
#include "fh_common.h"

namespace fh {

struct BNArgs {
    const float* x;
    float* y;
    const float* res;
    const float* dy;
    const float* yout;
    float* dx;
    float* dres;
    const float* gamma;
    const float* beta;
    float* rmean;
    float* rvar;
    float* save_mean;
    float* save_invstd;
    float* dgamma;
    float* dbeta;
    double* part;  // [z][C][SP][2]
    int SP;        // partial pairs per (client, channel) merge() adds (S, or conv tiles)
    int64_t x_cs, y_cs, res_cs, dy_cs, yo_cs, dx_cs, dres_cs, p_cs, r_cs, g_cs;
    const int32_t* counts;
    int batch, C, HW, S, chunk;  // chunk: elements per slice (multiple of 4)
    float eps, momentum;
    int relu;
    int vec;  // float4 element path (HW % 4 == 0; pooled input also needs W % 4 == 0)
    FastDiv fd_hw;
    // backward through a 2x2 max-pool (+dropout): dy is not materialised; the gradient
    // of element (img,c,y,x) is dpool[img,c,y/2,x/2] (x dropout keep/scale) routed by
    // the window argmax pidx (== (y&1)*2 + (x&1)), else 0
    const float* dpool;
    const uint8_t* pidx;
    const uint8_t* pmask;
    int64_t dp_cs, pi_cs, pm_cs;
    float pscale;
    int W;
    FastDiv fd_w;

    // host-side fills the entry points share (bn_args() sets the shape fields)
    void params(const float* gamma_, const float* beta_, int64_t p_cs_, float* rmean_,
                float* rvar_, int64_t r_cs_, float* save_mean_, float* save_invstd_, float eps_,
                float momentum_) {
        gamma = gamma_; beta = beta_; p_cs = p_cs_;
        rmean = rmean_; rvar = rvar_; r_cs = r_cs_;
        save_mean = save_mean_; save_invstd = save_invstd_;
        eps = eps_; momentum = momentum_;
    }
    void fwd_io(const float* x_, int64_t x_cs_, float* y_, int64_t y_cs_, const float* res_,
                int64_t res_cs_, int relu_) {
        x = x_; x_cs = x_cs_; y = y_; y_cs = y_cs_; res = res_; res_cs = res_cs_; relu = relu_;
    }
    void bwd_in(const float* x_, int64_t x_cs_, const float* gamma_, const float* beta_,
                int64_t p_cs_, const float* save_mean_, const float* save_invstd_, int relu_) {
        x = x_; x_cs = x_cs_; gamma = gamma_; beta = beta_; p_cs = p_cs_;
        save_mean = (float*)save_mean_; save_invstd = (float*)save_invstd_; relu = relu_;
    }
    void bwd_out(float* dx_, int64_t dx_cs_, float* dgamma_, float* dbeta_, int64_t g_cs_) {
        dx = dx_; dx_cs = dx_cs_; dgamma = dgamma_; dbeta = dbeta_; g_cs = g_cs_;
    }
    // the upstream gradient routed from a pooled one; its float4 path also needs W % 4 == 0
    void pool_route(const float* dpool_, int64_t dp_cs_, const uint8_t* pidx_, int64_t pi_cs_,
                    const uint8_t* pmask_, int64_t pm_cs_, float p_drop, int W_) {
        dpool = dpool_; pidx = pidx_; pmask = pmask_;
        dp_cs = dp_cs_; pi_cs = pi_cs_; pm_cs = pm_cs_;
        pscale = 1.0f / (1.0f - p_drop);
        W = W_;
        fd_w = FastDiv(W_);
        vec = (HW & 3) == 0 && (W_ & 3) == 0;
    }
    // partials from a convolution epilogue: one pair per 256-element tile of batch x elems
    void conv_tiles(const double* part_, int batch_, int elems) {
        part = (double*)part_;
        SP = (int)ceil_div((int64_t)batch_ * elems, 256);
    }
};

// Visit this block's slice of channel c of client z: f(offset_within_client_tensor, nvec)
// nvec = 4 (float4 at offset) or 1 (scalar).
template <class F>
__device__ __forceinline__ void for_slice(const BNArgs& a, int z, int c, int s, F&& f) {
    const int cnt = a.counts ? a.counts[z] : a.batch;
    const int n = cnt * a.HW;
    const int e0 = s * a.chunk, e1 = min(n, e0 + a.chunk);
    const int64_t istride = (int64_t)a.C * a.HW, coff = (int64_t)c * a.HW;
    if (a.vec) {
        for (int e = e0 + threadIdx.x * 4; e < e1; e += 256 * 4) {
            uint32_t img, p;
            a.fd_hw.divmod(e, img, p);
            f(img * istride + coff + p, 4);
        }
    } else {
        for (int e = e0 + threadIdx.x; e < e1; e += 256) {
            uint32_t img, p;
            a.fd_hw.divmod(e, img, p);
            f(img * istride + coff + p, 1);
        }
    }
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// Merge channel c's S partials -> (sum0, sum1), wave-cooperative: lane l adds partials
// l, l+64, ... in order, then an xor-shuffle tree; a fixed order, the same result in every
// lane.  Every lane of the calling wave must call it with the same (z, c).  (A sequential
// merge by one thread was S/8 dependent L2 round trips: the finalize on the critical path.)
__device__ __forceinline__ void merge(const BNArgs& a, int z, int c, double& s0, double& s1) {
    const double2* p = reinterpret_cast<const double2*>(a.part + (((int64_t)z * a.C + c) * a.SP) * 2);
    s0 = 0.0;
    s1 = 0.0;
    for (int i = threadIdx.x & 63; i < a.SP; i += 64) {
        const double2 v = p[i];
        s0 += v.x;
        s1 += v.y;
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
}

__global__ void __launch_bounds__(256) bn_stats_kernel(const BNArgs a) {
    __shared__ double red[4];
    const int s = blockIdx.x, c = blockIdx.y, z = blockIdx.z;
    const float* xz = a.x + z * a.x_cs;
    double s0 = 0.0, s1 = 0.0;
    for_slice(a, z, c, s, [&](int64_t o, int nv) {
        if (nv == 4) {
            const float4 v = ld4(xz + o);
            s0 += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
            s1 += ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
        } else {
            const double v = xz[o];
            s0 += v;
            s1 += v * v;
        }
    });
    s0 = block_sum_256(s0, red);
    s1 = block_sum_256(s1, red);
    if (threadIdx.x == 0) {
        double* p = a.part + ((((int64_t)z * a.C + c) * a.S) + s) * 2;
        p[0] = s0;
        p[1] = s1;
    }
}

// The train-mode finalize of channel c of client z, the one definition every forward kernel
// calls: the merged moments (sum, sq) over the client's n elements -> mean, clamped biased
// variance and invstd in fp64, cast to fp32; with `write`, save_mean / save_invstd and the
// running-statistics update (unbiased variance); returns alpha = invstd*w and
// beta' = b - mean*alpha.  The contract: a consumer that applies the returned affine on load,
// relu(x*scale + shift), is bit-identical to bn_apply_kernel's output, both taking alpha and
// beta' from these operations.
struct BNAffine {
    float alpha, bconst;
};

__device__ __forceinline__ BNAffine bn_finalize_channel(const BNArgs& a, int z, int c, int64_t n,
                                                        double sum, double sq, bool write) {
    const double mean = n > 0 ? sum / (double)n : 0.0;
    double var = n > 0 ? sq / (double)n - mean * mean : 0.0;
    if (var < 0.0) var = 0.0;
    const double invstd = n > 0 ? 1.0 / sqrt(var + (double)a.eps) : 0.0;
    const float meanf = (float)mean, invstdf = (float)invstd;
    if (write) {
        a.save_mean[z * a.C + c] = meanf;
        a.save_invstd[z * a.C + c] = invstdf;
        if (a.rmean && n > 0) {
            const double unb = n > 1 ? var * (double)n / (double)(n - 1) : var;
            float* rm = a.rmean + z * a.r_cs + c;
            float* rv = a.rvar + z * a.r_cs + c;
            *rm = (float)((double)a.momentum * mean + (1.0 - (double)a.momentum) * (double)*rm);
            *rv = (float)((double)a.momentum * unb + (1.0 - (double)a.momentum) * (double)*rv);
        }
    }
    const float alpha = invstdf * a.gamma[z * a.p_cs + c];
    return {alpha, a.beta[z * a.p_cs + c] - meanf * alpha};
}

__global__ void __launch_bounds__(256) bn_apply_kernel(const BNArgs a) {
    const int s = blockIdx.x, c = blockIdx.y, z = blockIdx.z;
    const int cnt = a.counts ? a.counts[z] : a.batch;
    const int64_t n = (int64_t)cnt * a.HW;
    double sum, sq;
    merge(a, z, c, sum, sq);
    // y = x*alpha + beta' [+res], [relu]
    const BNAffine f = bn_finalize_channel(a, z, c, n, sum, sq, s == 0 && threadIdx.x == 0);
    const float alpha = f.alpha, bconst = f.bconst;
    const float* xz = a.x + z * a.x_cs;
    float* yz = a.y + z * a.y_cs;
    const float* rz = a.res ? a.res + z * a.res_cs : nullptr;
    const int relu = a.relu;
    for_slice(a, z, c, s, [&](int64_t o, int nv) {
        if (nv == 4) {
            float4 v = ld4(xz + o);
            v.x = v.x * alpha + bconst;
            v.y = v.y * alpha + bconst;
            v.z = v.z * alpha + bconst;
            v.w = v.w * alpha + bconst;
            if (rz) {
                const float4 r = ld4(rz + o);
                v.x = v.x + r.x; v.y = v.y + r.y; v.z = v.z + r.z; v.w = v.w + r.w;
            }
            if (relu) {
                v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f);
                v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
            }
            st4(yz + o, v);
        } else {
            float v = xz[o] * alpha + bconst;
            if (rz) v = v + rz[o];
            if (relu) v = fmaxf(v, 0.f);
            yz[o] = v;
        }
    });
}

// Train-mode statistics without the apply pass: per (client, channel) the merged moments
// become save_mean / save_invstd, the running-stat update, and the affine the consumer
// applies on load (scale, shift = bn_finalize_channel's alpha, beta').
__global__ void __launch_bounds__(256) bn_finalize_kernel(const BNArgs a, float* scale,
                                                          float* shift, int64_t s_cs) {
    // one wave per channel (merge() is wave-cooperative)
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), z = blockIdx.y;
    if (c >= a.C) return;
    const int cnt = a.counts ? a.counts[z] : a.batch;
    const int64_t n = (int64_t)cnt * a.HW;
    double sum, sq;
    merge(a, z, c, sum, sq);
    if ((threadIdx.x & 63) != 0) return;
    const BNAffine f = bn_finalize_channel(a, z, c, n, sum, sq, true);
    scale[z * s_cs + c] = f.alpha;
    shift[z * s_cs + c] = f.bconst;
}

// BatchNorm finalize fused into the 2x2 max-pool (+dropout) that consumes the BN-ReLU output
// (CIFAR10CNN bn2/bn4/bn6 -> relu -> pool -> dropout, models_pytorch.py:139-155): one launch
// instead of fh_bn_finalize_tiles + fh_maxpool2_fwd_bnrelu.  Blocks own one channel of one
// client (BPC blocks per channel split its pooled elements); each merges the channel's
// per-tile partials from the producing conv's epilogue (lane-strided fp64 sums combined by
// xor-shuffles: a fixed order, the same in every block of the channel), derives the affine
// (bn_finalize_channel), and pools relu(x*alpha + beta') with maxpool2_fwd_kernel's tail
// (maxpool2_tail: window argmax, Philox keep-mask keyed by the pooled element index).
// Block 0 of the channel writes save_mean / save_invstd, the running statistics and the
// affine.
constexpr int kPoolEpt = 4;  // pooled elements per thread in maxpool2_bnfin_kernel

__global__ void __launch_bounds__(256)
maxpool2_bnfin_kernel(const BNArgs a, float* __restrict__ scale_out, float* __restrict__ shift_out,
                      int64_t s_cs, const float* __restrict__ x, int64_t x_cs,
                      float* __restrict__ y, int64_t y_cs, uint8_t* __restrict__ idx, int64_t i_cs,
                      uint8_t* __restrict__ mask, int64_t m_cs, int H, int W, int drop_mode,
                      float keep_prob, float dscale, uint64_t seed_salt,
                      const uint64_t* __restrict__ seed_dev, int bpc) {
    __shared__ float s_aff[2];
    const int z = blockIdx.y, c = blockIdx.x / bpc, sb = blockIdx.x - c * bpc;
    const int cnt = a.counts ? a.counts[z] : a.batch;
    const int64_t n = (int64_t)cnt * a.HW;
    // this thread's windows (kPoolEpt pooled elements, 256 apart: host
    // bpc = ceil(batch*ohw / (256*kPoolEpt))), loaded before the merge so the loads are in
    // flight across it and one merge serves kPoolEpt*256 elements
    const int OH = H / 2, OW = W / 2, ohw = OH * OW;
    const int64_t per_ch = (int64_t)cnt * ohw;
    int64_t e[kPoolEpt];
    float xv[kPoolEpt][4];
#pragma unroll
    for (int k = 0; k < kPoolEpt; ++k) {
        const int64_t q = ((int64_t)sb * kPoolEpt + k) * 256 + threadIdx.x;
        e[k] = -1;
        xv[k][0] = xv[k][1] = xv[k][2] = xv[k][3] = 0.f;
        if (q < per_ch) {
            const int img = (int)(q / ohw), r = (int)(q - (int64_t)img * ohw);
            const int oh = r / OW, ow = r - oh * OW;
            const int64_t plane = (int64_t)img * a.C + c;
            e[k] = plane * ohw + r;  // maxpool2_fwd_kernel's element index
            const float* pp = x + z * x_cs + plane * H * W + (2 * oh) * W + 2 * ow;
            xv[k][0] = pp[0]; xv[k][1] = pp[1]; xv[k][2] = pp[W]; xv[k][3] = pp[W + 1];
        }
    }
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        double s0, s1;
        merge(a, z, c, s0, s1);
        if (lane == 0) {
            const BNAffine f = bn_finalize_channel(a, z, c, n, s0, s1, sb == 0);
            s_aff[0] = f.alpha;
            s_aff[1] = f.bconst;
            if (sb == 0) {
                scale_out[z * s_cs + c] = f.alpha;
                shift_out[z * s_cs + c] = f.bconst;
            }
        }
    }
    __syncthreads();
    const float s = s_aff[0], t = s_aff[1];
    const uint64_t seed = seed_salt + (seed_dev ? *seed_dev : 0ull);
    const uint64_t prow = drop_mode == 1 ? philox_row(seed_dev, z) : 0ull;  // once, not per store
#pragma unroll
    for (int k = 0; k < kPoolEpt; ++k) {
        if (e[k] < 0) continue;
        const float v0 = fmaxf(xv[k][0] * s + t, 0.f), v1 = fmaxf(xv[k][1] * s + t, 0.f);
        const float v2 = fmaxf(xv[k][2] * s + t, 0.f), v3 = fmaxf(xv[k][3] * s + t, 0.f);
        y[z * y_cs + e[k]] = maxpool2_tail(v0, v1, v2, v3, z, e[k], idx, i_cs, mask, m_cs, drop_mode,
                                           keep_prob, dscale, seed, prow);
    }
}

// eval mode: running statistics (LocalTrainer._validate_epoch / evaluate_model)
__global__ void __launch_bounds__(256) bn_eval_kernel(const BNArgs a) {
    const int s = blockIdx.x, c = blockIdx.y, z = blockIdx.z;
    const float invstd = (float)(1.0 / sqrt((double)a.rvar[z * a.r_cs + c] + (double)a.eps));
    const float alpha = invstd * a.gamma[z * a.p_cs + c];
    const float bconst = a.beta[z * a.p_cs + c] - a.rmean[z * a.r_cs + c] * alpha;
    const float* xz = a.x + z * a.x_cs;
    float* yz = a.y + z * a.y_cs;
    const float* rz = a.res ? a.res + z * a.res_cs : nullptr;
    for_slice(a, z, c, s, [&](int64_t o, int nv) {
        for (int q = 0; q < nv; ++q) {
            float v = xz[o + q] * alpha + bconst;
            if (rz) v = v + rz[o + q];
            if (a.relu) v = fmaxf(v, 0.f);
            yz[o + q] = v;
        }
    });
}


// upstream gradient at client-tensor offset o (before the ReLU mask): dy[o], or routed
// from the pooled gradient (maxpool2_bwd semantics, layers.hip)
__device__ __forceinline__ float pooled_g(const BNArgs& a, int z, int64_t o) {
    uint32_t y, x;
    const int64_t plane = o / a.HW;  // img*C + c
    a.fd_w.divmod((uint32_t)(o - plane * a.HW), y, x);
    const int64_t e = plane * (a.HW >> 2) + (int64_t)(y >> 1) * (a.W >> 1) + (x >> 1);
    if (a.pidx[z * a.pi_cs + e] != (int)(((y & 1) << 1) | (x & 1))) return 0.f;
    float g = a.dpool[z * a.dp_cs + e];
    if (a.pmask) g = a.pmask[z * a.pm_cs + e] ? g * a.pscale : 0.f;
    return g;
}

__device__ __forceinline__ float4 upstream4(const BNArgs& a, int z, int64_t o) {
    if (!a.dpool) return ld4(a.dy + z * a.dy_cs + o);
    // 4 consecutive columns (x % 4 == 0) = 2 pooled windows of one pooled row
    uint32_t y, x;
    const int64_t plane = o / a.HW;
    a.fd_w.divmod((uint32_t)(o - plane * a.HW), y, x);
    const int64_t e = plane * (a.HW >> 2) + (int64_t)(y >> 1) * (a.W >> 1) + (x >> 1);
    const int r = (y & 1) << 1;
    // every load unconditional (a null keep-mask reads the argmax bytes) and each keep byte
    // folded into its argmax code, which every result uses: r05 — under `if (pmask)` each mask
    // byte's load and use sat in a branch of their own, a dependent round trip per byte
    const uint8_t* pk = a.pmask ? a.pmask + z * a.pm_cs : a.pidx + z * a.pi_cs;
    float g0 = a.dpool[z * a.dp_cs + e], g1 = a.dpool[z * a.dp_cs + e + 1];
    const int c0 = a.pidx[z * a.pi_cs + e] | (pk[e] ? 4 : 0);
    const int c1 = a.pidx[z * a.pi_cs + e + 1] | (pk[e + 1] ? 4 : 0);
    const bool dm = a.pmask != nullptr;
    const float h0 = dm ? g0 * a.pscale : g0, h1 = dm ? g1 * a.pscale : g1;
    g0 = (!dm || (c0 & 4)) ? h0 : 0.f;
    g1 = (!dm || (c1 & 4)) ? h1 : 0.f;
    const int i0 = c0 & 3, i1 = c1 & 3;
    return make_float4(i0 == r ? g0 : 0.f, i0 == (r | 1) ? g0 : 0.f, i1 == r ? g1 : 0.f,
                       i1 == (r | 1) ? g1 : 0.f);
}

__device__ __forceinline__ float upstream1(const BNArgs& a, int z, int64_t o) {
    return a.dpool ? pooled_g(a, z, o) : a.dy[z * a.dy_cs + o];
}

// ReLU mask of the backward: from the stored forward output (yout > 0), or — no residual
// add in between — recomputed from x exactly as the forward evaluated it
// (x*alpha + beta' > 0 with the same fp32 operations), which saves reading yout.
struct ReluMask {
    int mode;  // 0 none, 1 yout, 2 recompute
    const float* yo;
    float alpha, bconst;
    __device__ ReluMask(const BNArgs& a, int z, int c, float mean, float invstd) {
        mode = !a.relu ? 0 : (a.yout ? 1 : 2);
        yo = mode == 1 ? a.yout + z * a.yo_cs : nullptr;
        alpha = 0.f;
        bconst = 0.f;
        if (mode == 2) {
            alpha = invstd * a.gamma[z * a.p_cs + c];
            bconst = a.beta[z * a.p_cs + c] - mean * alpha;
        }
    }
    __device__ __forceinline__ bool keep(float x, int64_t o) const {
        if (mode == 0) return true;
        if (mode == 1) return yo[o] > 0.f;
        return x * alpha + bconst > 0.f;
    }
    __device__ __forceinline__ float4 apply4(float4 g, float4 xv, int64_t o) const {
        if (mode == 0) return g;
        float4 m;
        if (mode == 1) {
            m = ld4(yo + o);
        } else {
            m.x = xv.x * alpha + bconst; m.y = xv.y * alpha + bconst;
            m.z = xv.z * alpha + bconst; m.w = xv.w * alpha + bconst;
        }
        g.x = m.x > 0.f ? g.x : 0.f; g.y = m.y > 0.f ? g.y : 0.f;
        g.z = m.z > 0.f ? g.z : 0.f; g.w = m.w > 0.f ? g.w : 0.f;
        return g;
    }
};

__global__ void __launch_bounds__(256) bn_bwd_reduce_kernel(const BNArgs a) {
    __shared__ double red[4];
    const int s = blockIdx.x, c = blockIdx.y, z = blockIdx.z;
    const float mean = a.save_mean[z * a.C + c], invstd = a.save_invstd[z * a.C + c];
    const ReluMask rm(a, z, c, mean, invstd);
    const float* xz = a.x + z * a.x_cs;
    float* drz = a.dres ? a.dres + z * a.dres_cs : nullptr;
    double sg = 0.0, dot = 0.0;
    for_slice(a, z, c, s, [&](int64_t o, int nv) {
        if (nv == 4) {
            const float4 xv = ld4(xz + o);
            const float4 g = rm.apply4(upstream4(a, z, o), xv, o);
            if (drz) st4(drz + o, g);
            sg += ((double)g.x + (double)g.y) + ((double)g.z + (double)g.w);
            dot += ((double)((xv.x - mean) * g.x) + (double)((xv.y - mean) * g.y)) +
                   ((double)((xv.z - mean) * g.z) + (double)((xv.w - mean) * g.w));
        } else {
            const float xv = xz[o];
            const float g = rm.keep(xv, o) ? upstream1(a, z, o) : 0.f;
            if (drz) drz[o] = g;
            sg += (double)g;
            dot += (double)((xv - mean) * g);
        }
    });
    sg = block_sum_256(sg, red);
    dot = block_sum_256(dot, red);
    if (threadIdx.x == 0) {
        double* p = a.part + ((((int64_t)z * a.C + c) * a.S) + s) * 2;
        p[0] = sg;
        p[1] = dot;
    }
}

__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(const BNArgs a) {
    const int s = blockIdx.x, c = blockIdx.y, z = blockIdx.z;
    const int cnt = a.counts ? a.counts[z] : a.batch;
    const int64_t n = (int64_t)cnt * a.HW;
    double sg, dot;
    merge(a, z, c, sg, dot);
    const float mean = a.save_mean[z * a.C + c], invstd = a.save_invstd[z * a.C + c];
    if (s == 0 && threadIdx.x == 0) {
        if (a.dgamma) a.dgamma[z * a.g_cs + c] = (float)(dot * (double)invstd);
        if (a.dbeta) a.dbeta[z * a.g_cs + c] = (float)sg;
    }
    if (!a.dx) return;
    const ReluMask rm(a, z, c, mean, invstd);
    const float w = a.gamma[z * a.p_cs + c];
    const float k = n > 0 ? (float)(dot * (double)invstd * (double)invstd / (double)n) : 0.f;
    const float gm = n > 0 ? (float)(sg / (double)n) : 0.f;
    const float* xz = a.x + z * a.x_cs;
    float* dxz = a.dx + z * a.dx_cs;
    auto apply4 = [&](float4 g, float4 xv) {
        float4 r;
        r.x = (((g.x - gm) - (xv.x - mean) * k) * invstd) * w;
        r.y = (((g.y - gm) - (xv.y - mean) * k) * invstd) * w;
        r.z = (((g.z - gm) - (xv.z - mean) * k) * invstd) * w;
        r.w = (((g.w - gm) - (xv.w - mean) * k) * invstd) * w;
        return r;
    };
    if (a.vec) {
        // float4 path, two element quads per thread per iteration with every load issued
        // before the first store (dx may alias nothing the loop reads, but the compiler
        // cannot know: one quad per iteration left one HBM round trip per quad)
        const int e0 = s * a.chunk, e1 = min((int)n, e0 + a.chunk);
        const int64_t istride = (int64_t)a.C * a.HW, coff = (int64_t)c * a.HW;
        for (int e = e0 + threadIdx.x * 4; e < e1; e += 2 * 256 * 4) {
            const bool two = e + 256 * 4 < e1;
            uint32_t img, p;
            a.fd_hw.divmod(e, img, p);
            const int64_t oa = img * istride + coff + p;
            int64_t ob = oa;
            if (two) {
                a.fd_hw.divmod(e + 256 * 4, img, p);
                ob = img * istride + coff + p;
            }
            const float4 xa = ld4(xz + oa), xb = ld4(xz + ob);
            const float4 ua = upstream4(a, z, oa), ub = upstream4(a, z, ob);
            const float4 ra = apply4(rm.apply4(ua, xa, oa), xa);
            const float4 rb = apply4(rm.apply4(ub, xb, ob), xb);
            st4(dxz + oa, ra);
            if (two) st4(dxz + ob, rb);
        }
        return;
    }
    for_slice(a, z, c, s, [&](int64_t o, int nv) {
        if (nv == 4) {
            const float4 xv = ld4(xz + o);
            const float4 g = rm.apply4(upstream4(a, z, o), xv, o);
            st4(dxz + o, apply4(g, xv));
        } else {
            const float xv = xz[o];
            const float g = rm.keep(xv, o) ? upstream1(a, z, o) : 0.f;
            dxz[o] = (((g - gm) - (xv - mean) * k) * invstd) * w;
        }
    });
}

static void bn_geometry(int nclients, int batch, int C, int HW, int& S, int& chunk) {
    const int64_t nmax = (int64_t)batch * HW;
    int64_t want = ceil_div(2048, (int64_t)C * std::max(nclients, 1));
    const int64_t maxs = std::max<int64_t>(1, nmax / 2048);  // >= 2048 elements per slice
    if (want > maxs) want = maxs;
    if (want < 1) want = 1;
    chunk = (int)(ceil_div(ceil_div(nmax, want), 4) * 4);
    S = (int)ceil_div(nmax, chunk);
}

static BNArgs bn_args(int nclients, int batch, int C, int HW, const int32_t* counts) {
    BNArgs a{};
    a.counts = counts;
    a.batch = batch;
    a.C = C;
    a.HW = HW;
    bn_geometry(nclients, batch, C, HW, a.S, a.chunk);
    a.SP = a.S;
    a.fd_hw = FastDiv(HW);
    a.vec = (HW & 3) == 0;
    return a;
}

// the backward's two passes over a.S slices (fh_bn_bwd, fh_bn_bwd_pool)
static int bn_bwd_launch(const BNArgs& a, int nclients, void* stream, const char* reduce_name,
                         const char* apply_name) {
    hipStream_t st = as_stream(stream);
    dim3 grid(a.S, a.C, nclients);
    FH_LAUNCH(bn_bwd_reduce_kernel, grid, dim3(256), 0, st, a);
    FH_LAUNCH_CHECK(reduce_name);
    FH_LAUNCH(bn_bwd_apply_kernel, grid, dim3(256), 0, st, a);
    FH_LAUNCH_CHECK(apply_name);
    return FH_OK;
}

}  // namespace fh

using namespace fh;

extern "C" size_t fh_bn_workspace(int32_t nclients, int32_t batch, int32_t C, int32_t HW) {
    if (nclients <= 0 || batch <= 0 || C <= 0 || HW <= 0) return 0;
    int S, chunk;
    bn_geometry(nclients, batch, C, HW, S, chunk);
    return (size_t)nclients * C * S * 2 * sizeof(double);
}

extern "C" int fh_bn_fwd_train(const float* x, int64_t x_cs, float* y, int64_t y_cs,
                               const float* res, int64_t res_cs, const float* gamma,
                               const float* beta, int64_t p_cs, float* running_mean,
                               float* running_var, int64_t r_cs, float* save_mean,
                               float* save_invstd, const int32_t* counts, int32_t nclients,
                               int32_t batch, int32_t C, int32_t HW, float eps, float momentum,
                               int32_t relu, void* workspace, size_t ws_bytes, void* stream) {
    FH_REQUIRE(nclients >= 0 && batch > 0 && C > 0 && HW > 0, "bn_fwd_train: bad shape");
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(x && y && gamma && beta && save_mean && save_invstd, "bn_fwd_train: null pointer");
    FH_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bn_fwd_train: running stats");
    const size_t need = fh_bn_workspace(nclients, batch, C, HW);
    FH_REQUIRE(workspace && ws_bytes >= need, "bn_fwd_train: workspace %zu < %zu", ws_bytes, need);
    BNArgs a = bn_args(nclients, batch, C, HW, counts);
    a.fwd_io(x, x_cs, y, y_cs, res, res_cs, relu);
    a.params(gamma, beta, p_cs, running_mean, running_var, r_cs, save_mean, save_invstd, eps,
             momentum);
    a.part = (double*)workspace;
    hipStream_t st = as_stream(stream);
    dim3 grid(a.S, C, nclients);
    FH_LAUNCH(bn_stats_kernel, grid, dim3(256), 0, st, a);
    FH_LAUNCH_CHECK("bn_fwd_train stats");
    FH_LAUNCH(bn_apply_kernel, grid, dim3(256), 0, st, a);
    FH_LAUNCH_CHECK("bn_fwd_train apply");
    return FH_OK;
}

extern "C" int fh_bn_fwd_stats(const float* x, int64_t x_cs, const float* gamma,
                               const float* beta, int64_t p_cs, float* running_mean,
                               float* running_var, int64_t r_cs, float* save_mean,
                               float* save_invstd, float* scale_out, float* shift_out,
                               int64_t s_cs, const int32_t* counts, int32_t nclients,
                               int32_t batch, int32_t C, int32_t HW, float eps, float momentum,
                               void* workspace, size_t ws_bytes, void* stream) {
    FH_REQUIRE(nclients >= 0 && batch > 0 && C > 0 && HW > 0, "bn_fwd_stats: bad shape");
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(x && gamma && beta && save_mean && save_invstd && scale_out && shift_out,
               "bn_fwd_stats: null pointer");
    FH_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bn_fwd_stats: running stats");
    const size_t need = fh_bn_workspace(nclients, batch, C, HW);
    FH_REQUIRE(workspace && ws_bytes >= need, "bn_fwd_stats: workspace %zu < %zu", ws_bytes, need);
    BNArgs a = bn_args(nclients, batch, C, HW, counts);
    a.x = x;
    a.x_cs = x_cs;
    a.params(gamma, beta, p_cs, running_mean, running_var, r_cs, save_mean, save_invstd, eps,
             momentum);
    a.part = (double*)workspace;
    hipStream_t st = as_stream(stream);
    FH_LAUNCH(bn_stats_kernel, dim3(a.S, C, nclients), dim3(256), 0, st, a);
    FH_LAUNCH_CHECK("bn_fwd_stats stats");
    FH_LAUNCH(bn_finalize_kernel, dim3((unsigned)ceil_div(C, 4), nclients), dim3(256), 0,
                       st, a, scale_out, shift_out, s_cs);
    FH_LAUNCH_CHECK("bn_fwd_stats finalize");
    return FH_OK;
}

// Train-mode statistics from partials a convolution epilogue already wrote
// (fh_conv2d_fwd_bnstats: one fp64 (sum, sum of squares) pair per (client, channel,
// 256-pixel tile), zeros past a client's count): bn_finalize_kernel merges the tiles in
// order -> save_mean / save_invstd, running statistics, and the consumer's affine.
extern "C" int fh_bn_finalize_tiles(const double* part, const float* gamma, const float* beta,
                                    int64_t p_cs, float* running_mean, float* running_var,
                                    int64_t r_cs, float* save_mean, float* save_invstd,
                                    float* scale_out, float* shift_out, int64_t s_cs,
                                    const int32_t* counts, int32_t nclients, int32_t batch,
                                    int32_t C, int32_t HW, float eps, float momentum,
                                    void* stream) {
    FH_REQUIRE(nclients >= 0 && batch > 0 && C > 0 && HW > 0, "bn_finalize_tiles: bad shape");
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(part && gamma && beta && save_mean && save_invstd && scale_out && shift_out,
               "bn_finalize_tiles: null pointer");
    FH_REQUIRE((running_mean == nullptr) == (running_var == nullptr),
               "bn_finalize_tiles: running stats");
    BNArgs a = bn_args(nclients, batch, C, HW, counts);
    a.conv_tiles(part, batch, HW);
    a.params(gamma, beta, p_cs, running_mean, running_var, r_cs, save_mean, save_invstd, eps,
             momentum);
    FH_LAUNCH(bn_finalize_kernel, dim3((unsigned)ceil_div(C, 4), nclients), dim3(256), 0,
              as_stream(stream), a, scale_out, shift_out, s_cs);
    FH_LAUNCH_CHECK("bn_finalize_tiles");
    return FH_OK;
}

// fh_bn_fwd_train's apply pass from the per-tile statistics a convolution epilogue wrote
// (FederatedResNet's stem bn1 and block bn2, whose output is materialised because the next
// block reads it twice, conv and residual): bn_apply_kernel merges the conv tiles instead of
// bn_stats_kernel's slices -> y = [relu](x*alpha + beta' [+ res]), save_mean / save_invstd
// and the running statistics.  y is never re-read for its statistics.
extern "C" int fh_bn_apply_tiles(const double* part, const float* x, int64_t x_cs, float* y,
                                 int64_t y_cs, const float* res, int64_t res_cs,
                                 const float* gamma, const float* beta, int64_t p_cs,
                                 float* running_mean, float* running_var, int64_t r_cs,
                                 float* save_mean, float* save_invstd, const int32_t* counts,
                                 int32_t nclients, int32_t batch, int32_t C, int32_t HW,
                                 float eps, float momentum, int32_t relu, void* stream) {
    FH_REQUIRE(nclients >= 0 && batch > 0 && C > 0 && HW > 0, "bn_apply_tiles: bad shape");
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(part && x && y && gamma && beta && save_mean && save_invstd,
               "bn_apply_tiles: null pointer");
    FH_REQUIRE((running_mean == nullptr) == (running_var == nullptr),
               "bn_apply_tiles: running stats");
    BNArgs a = bn_args(nclients, batch, C, HW, counts);
    a.conv_tiles(part, batch, HW);
    a.fwd_io(x, x_cs, y, y_cs, res, res_cs, relu);
    a.params(gamma, beta, p_cs, running_mean, running_var, r_cs, save_mean, save_invstd, eps,
             momentum);
    FH_LAUNCH(bn_apply_kernel, dim3(a.S, C, nclients), dim3(256), 0, as_stream(stream), a);
    FH_LAUNCH_CHECK("bn_apply_tiles");
    return FH_OK;
}

// fh_bn_finalize_tiles + fh_maxpool2_fwd_bnrelu in one launch (maxpool2_bnfin_kernel).
extern "C" int fh_maxpool2_fwd_bnfinalize(
        const double* part, const float* gamma, const float* beta, int64_t p_cs,
        float* running_mean, float* running_var, int64_t r_cs, float* save_mean,
        float* save_invstd, float* scale_out, float* shift_out, int64_t s_cs, const float* x,
        int64_t x_cs, float* y, int64_t y_cs, uint8_t* idx, int64_t i_cs, uint8_t* mask,
        int64_t m_cs, const int32_t* counts, int32_t nclients, int32_t batch, int32_t C,
        int32_t H, int32_t W, float eps, float momentum, int32_t drop_mode, float p_drop,
        uint64_t seed, const uint64_t* seed_dev, void* stream) {
    FH_REQUIRE(nclients >= 0 && batch > 0 && C > 0 && H >= 2 && W >= 2 && !(H & 1) && !(W & 1),
               "maxpool2_fwd_bnfinalize: bad shape");
    FH_REQUIRE(drop_mode >= 0 && drop_mode <= 2 && (drop_mode == 0 || mask),
               "maxpool2_fwd_bnfinalize: mask");
    FH_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "maxpool2_fwd_bnfinalize: p=%g", p_drop);
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(part && gamma && beta && save_mean && save_invstd && scale_out && shift_out && x &&
               y && idx, "maxpool2_fwd_bnfinalize: null pointer");
    FH_REQUIRE((running_mean == nullptr) == (running_var == nullptr),
               "maxpool2_fwd_bnfinalize: running stats");
    BNArgs a = bn_args(nclients, batch, C, H * W, counts);
    a.conv_tiles(part, batch, H * W);
    a.params(gamma, beta, p_cs, running_mean, running_var, r_cs, save_mean, save_invstd, eps,
             momentum);
    const int64_t per_ch = (int64_t)batch * (H / 2) * (W / 2);
    const int bpc = (int)std::max<int64_t>(1, ceil_div(per_ch, 256 * kPoolEpt));
    const float keep = 1.0f - p_drop;
    FH_LAUNCH(maxpool2_bnfin_kernel, dim3((unsigned)(C * bpc), nclients), dim3(256), 0,
              as_stream(stream), a, scale_out, shift_out, s_cs, x, x_cs, y, y_cs, idx, i_cs,
              mask, m_cs, H, W, drop_mode, keep, 1.0f / keep, seed, seed_dev, bpc);
    FH_LAUNCH_CHECK("maxpool2_fwd_bnfinalize");
    return FH_OK;
}

extern "C" int fh_bn_fwd_eval(const float* x, int64_t x_cs, float* y, int64_t y_cs,
                              const float* res, int64_t res_cs, const float* gamma,
                              const float* beta, int64_t p_cs, const float* running_mean,
                              const float* running_var, int64_t r_cs, const int32_t* counts,
                              int32_t nclients, int32_t batch, int32_t C, int32_t HW, float eps,
                              int32_t relu, void* stream) {
    FH_REQUIRE(nclients >= 0 && batch > 0 && C > 0 && HW > 0, "bn_fwd_eval: bad shape");
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(x && y && gamma && beta && running_mean && running_var, "bn_fwd_eval: null pointer");
    BNArgs a = bn_args(nclients, batch, C, HW, counts);
    a.fwd_io(x, x_cs, y, y_cs, res, res_cs, relu);
    a.params(gamma, beta, p_cs, (float*)running_mean, (float*)running_var, r_cs, nullptr, nullptr,
             eps, 0.f);
    FH_LAUNCH(bn_eval_kernel, dim3(a.S, C, nclients), dim3(256), 0, as_stream(stream), a);
    FH_LAUNCH_CHECK("bn_fwd_eval");
    return FH_OK;
}

extern "C" int fh_bn_bwd(const float* dy, int64_t dy_cs, const float* yout, int64_t yo_cs,
                         const float* x, int64_t x_cs, const float* gamma, const float* beta,
                         int64_t p_cs,
                         const float* save_mean, const float* save_invstd, float* dx,
                         int64_t dx_cs, float* dres, int64_t dres_cs, float* dgamma, float* dbeta,
                         int64_t g_cs, const int32_t* counts, int32_t nclients, int32_t batch,
                         int32_t C, int32_t HW, int32_t relu, void* workspace, size_t ws_bytes,
                         void* stream) {
    FH_REQUIRE(nclients >= 0 && batch > 0 && C > 0 && HW > 0, "bn_bwd: bad shape");
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(dy && x && gamma && save_mean && save_invstd, "bn_bwd: null pointer");
    FH_REQUIRE(!relu || yout || beta, "bn_bwd: relu needs the forward output or beta");
    const size_t need = fh_bn_workspace(nclients, batch, C, HW);
    FH_REQUIRE(workspace && ws_bytes >= need, "bn_bwd: workspace %zu < %zu", ws_bytes, need);
    BNArgs a = bn_args(nclients, batch, C, HW, counts);
    a.dy = dy; a.dy_cs = dy_cs; a.yout = yout; a.yo_cs = yo_cs;
    a.dres = dres; a.dres_cs = dres_cs;
    a.bwd_in(x, x_cs, gamma, beta, p_cs, save_mean, save_invstd, relu);
    a.bwd_out(dx, dx_cs, dgamma, dbeta, g_cs);
    a.part = (double*)workspace;
    return bn_bwd_launch(a, nclients, stream, "bn_bwd reduce", "bn_bwd apply");
}

// BN backward whose upstream gradient arrives through MaxPool2d(2,2) (+ the Dropout fused
// after it): the full-resolution gradient is routed on the fly from dpool / pidx / pmask
// (maxpool2_bwd semantics) instead of being written and re-read.
extern "C" int fh_bn_bwd_pool(const float* dpool, int64_t dp_cs, const uint8_t* pidx,
                              int64_t pi_cs, const uint8_t* pmask, int64_t pm_cs, float p_drop,
                              const float* yout, int64_t yo_cs, const float* x, int64_t x_cs,
                              const float* gamma, const float* beta, int64_t p_cs,
                              const float* save_mean,
                              const float* save_invstd, float* dx, int64_t dx_cs, float* dgamma,
                              float* dbeta, int64_t g_cs, const int32_t* counts,
                              int32_t nclients, int32_t batch, int32_t C, int32_t H, int32_t W,
                              int32_t relu, void* workspace, size_t ws_bytes, void* stream) {
    FH_REQUIRE(nclients >= 0 && batch > 0 && C > 0 && H >= 2 && W >= 2 && !(H & 1) && !(W & 1),
               "bn_bwd_pool: bad shape");
    FH_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "bn_bwd_pool: p=%g", p_drop);
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(dpool && pidx && x && gamma && save_mean && save_invstd, "bn_bwd_pool: null pointer");
    FH_REQUIRE(!relu || yout || beta, "bn_bwd_pool: relu needs the forward output or beta");
    const int HW = H * W;
    const size_t need = fh_bn_workspace(nclients, batch, C, HW);
    FH_REQUIRE(workspace && ws_bytes >= need, "bn_bwd_pool: workspace %zu < %zu", ws_bytes, need);
    BNArgs a = bn_args(nclients, batch, C, HW, counts);
    a.pool_route(dpool, dp_cs, pidx, pi_cs, pmask, pm_cs, p_drop, W);
    a.yout = yout; a.yo_cs = yo_cs;
    a.bwd_in(x, x_cs, gamma, beta, p_cs, save_mean, save_invstd, relu);
    a.bwd_out(dx, dx_cs, dgamma, dbeta, g_cs);
    a.part = (double*)workspace;
    return bn_bwd_launch(a, nclients, stream, "bn_bwd_pool reduce", "bn_bwd_pool apply");
}

// BN backward from statistics a convolution's DGRAD epilogue already took
// (fh_conv2d_dgrad_bnstats: g is the ReLU-masked gradient, bn_part holds one fp64
// (sum g, sum (x - mean) g) pair per (client, channel, 256-pixel tile)): the apply pass of
// fh_bn_bwd only — dgamma / dbeta and dx = ((g - mean g) - (x - mean) k) invstd w.
extern "C" int fh_bn_bwd_tiles(const double* part, const float* g, int64_t g_cs_, const float* x,
                               int64_t x_cs, const float* gamma, int64_t p_cs,
                               const float* save_mean, const float* save_invstd, float* dx,
                               int64_t dx_cs, float* dgamma, float* dbeta, int64_t dg_cs,
                               const int32_t* counts, int32_t nclients, int32_t batch, int32_t C,
                               int32_t HW, void* stream) {
    FH_REQUIRE(nclients >= 0 && batch > 0 && C > 0 && HW > 0, "bn_bwd_tiles: bad shape");
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(part && g && x && gamma && save_mean && save_invstd, "bn_bwd_tiles: null pointer");
    BNArgs a = bn_args(nclients, batch, C, HW, counts);
    a.conv_tiles(part, batch, HW);
    a.dy = g; a.dy_cs = g_cs_;
    a.bwd_in(x, x_cs, gamma, nullptr, p_cs, save_mean, save_invstd, /*relu=*/0);  // g is masked
    a.bwd_out(dx, dx_cs, dgamma, dbeta, dg_cs);
    FH_LAUNCH(bn_bwd_apply_kernel, dim3(a.S, C, nclients), dim3(256), 0, as_stream(stream), a);
    FH_LAUNCH_CHECK("bn_bwd_tiles");
    return FH_OK;
}

// fh_bn_bwd_pool's apply pass from the partials fh_conv2d_dgrad_bnstats took with pidx (the
// statistics over the pooled grid's tiles, routed to the window argmax): dgamma / dbeta and
// dx, the gradient routed from dpool / pidx / pmask and the ReLU mask recomputed from x.
extern "C" int fh_bn_bwd_pool_tiles(const double* part, const float* dpool, int64_t dp_cs,
                                    const uint8_t* pidx, int64_t pi_cs, const uint8_t* pmask,
                                    int64_t pm_cs, float p_drop, const float* x, int64_t x_cs,
                                    const float* gamma, const float* beta, int64_t p_cs,
                                    const float* save_mean, const float* save_invstd, float* dx,
                                    int64_t dx_cs, float* dgamma, float* dbeta, int64_t g_cs,
                                    const int32_t* counts, int32_t nclients, int32_t batch,
                                    int32_t C, int32_t H, int32_t W, void* stream) {
    FH_REQUIRE(nclients >= 0 && batch > 0 && C > 0 && H >= 2 && W >= 2 && !(H & 1) && !(W & 1),
               "bn_bwd_pool_tiles: bad shape");
    FH_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "bn_bwd_pool_tiles: p=%g", p_drop);
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(part && dpool && pidx && x && gamma && beta && save_mean && save_invstd,
               "bn_bwd_pool_tiles: null pointer");
    const int HW = H * W;
    BNArgs a = bn_args(nclients, batch, C, HW, counts);
    a.conv_tiles(part, batch, HW / 4);  // the pooled grid's tiles
    a.pool_route(dpool, dp_cs, pidx, pi_cs, pmask, pm_cs, p_drop, W);
    a.bwd_in(x, x_cs, gamma, beta, p_cs, save_mean, save_invstd, /*relu=*/1);
    a.bwd_out(dx, dx_cs, dgamma, dbeta, g_cs);
    FH_LAUNCH(bn_bwd_apply_kernel, dim3(a.S, C, nclients), dim3(256), 0, as_stream(stream), a);
    FH_LAUNCH_CHECK("bn_bwd_pool_tiles");
    return FH_OK;
}
