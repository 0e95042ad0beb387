// optim_elem.h — the per-element optimizer updates, shared by the optimizer launches
// (optim.hip) and the linear weight-gradient epilogue that applies the update where the
// gradient is produced (conv.hip, linear_wgrad_skinny_body).  One copy: every user gives the
// same bits for the same (p, g, state).
//
// The rounding sequence follows ATen's CPU kernels for torch.optim's single-tensor path:
//   add(.., alpha)  -> fmadd(b, alpha, a)     lerp (w<.5) -> fmadd(w, e-s, s)
//   addcmul         -> a + (v*b)*c            addcdiv     -> a + v*(b/c)
#pragma once

#include "fh_common.h"

namespace fh {

__device__ __forceinline__ float sgd_elem(float pv, float gv, float bv, float neg_lr, float mom,
                                          float wd, int first, float& b_out) {
    if (wd != 0.f) gv = fmaf(pv, wd, gv);
    float b = gv;
    if (mom != 0.f) b = first ? gv : (bv * mom + gv);
    b_out = b;
    return fmaf(b, neg_lr, pv);
}

// One Adam/AdamW element in torch.optim's rounding order.
__device__ __forceinline__ float adam_elem(float pv, float gv, float& m, float& v, float wd,
                                          float decay_mul, int decoupled, float one_m_b1,
                                          float b2, float one_m_b2, float bc2_sqrt, float eps,
                                          float neg_step_size) {
    if (wd != 0.f) {
        if (decoupled) pv = pv * decay_mul;
        else gv = fmaf(pv, wd, gv);
    }
    const float mv = fmaf(one_m_b1, gv - m, m);
    const float vv = v * b2 + (one_m_b2 * gv) * gv;
    m = mv;
    v = vv;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    return pv + neg_step_size * (mv / denom);
}

struct OptScal {  // SGD: neg_lr, mom, wd, first | Adam: the adam_elem scalars
    float neg_lr, mom, wd;
    int first;
    float decay_mul, one_m_b1, b2, one_m_b2, bc2_sqrt, eps, neg_step_size;
    int decoupled;
    const float* scal;  // Adam: device {bc2_sqrt, -step_size} or null
};

// The host scalars in fp32, rounded where ATen meets the fp32 tensor (one place: the
// optimizer launches and the fused linear update must agree bit for bit).
inline OptScal sgd_scalars(float lr, float momentum, float weight_decay, int first_step) {
    OptScal o{};
    o.neg_lr = -lr;
    o.mom = momentum;
    o.wd = weight_decay;
    o.first = first_step;
    return o;
}
inline OptScal adam_scalars(double lr, double beta1, double beta2, double eps, double weight_decay,
                            int decoupled, double step_size, double bc2_sqrt,
                            const float* scal_dev) {
    OptScal o{};
    o.wd = (float)weight_decay;
    o.decay_mul = (float)(1.0 - lr * weight_decay);
    o.decoupled = decoupled;
    o.one_m_b1 = (float)(1.0 - beta1);
    o.b2 = (float)beta2;
    o.one_m_b2 = (float)(1.0 - beta2);
    o.bc2_sqrt = (float)bc2_sqrt;
    o.eps = (float)eps;
    o.neg_step_size = (float)(-step_size);
    o.scal = scal_dev;
    return o;
}

// The update of one float4 in two phases: opt_load4 issues its loads (p and the state, from
// in-bounds addresses — a missing momentum buffer reads p — so no load sits under a branch),
// opt_apply4 computes and stores.  The plain ranges load all their float4s first (r05: with
// the momentum load under `if (use_buf)` each float4's loads and update were one dependent
// round trip).
struct OptIn {
    float4 p, m, v;
};
template <bool ADAM>
__device__ __forceinline__ void opt_load4(const float4* p, const float4* s1, const float4* s2,
                                          int64_t i, OptIn& in) {
    in.p = p[i];
    in.m = (s1 ? s1 : p)[i];
    if constexpr (ADAM) in.v = s2[i];
}

template <bool ADAM>
__device__ __forceinline__ void opt_apply4(float4* p, float4* s1, float4* s2, int64_t i,
                                           const OptIn& in, float4 gv, const OptScal& o,
                                           float bc2_sqrt, float neg_step) {
    const float4 pv = in.p;
    float4 out;
    if constexpr (!ADAM) {
        const bool use_buf = o.mom != 0.f;
        const float4 bv = (use_buf && !o.first) ? in.m : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 b;
        out.x = sgd_elem(pv.x, gv.x, bv.x, o.neg_lr, o.mom, o.wd, o.first, b.x);
        out.y = sgd_elem(pv.y, gv.y, bv.y, o.neg_lr, o.mom, o.wd, o.first, b.y);
        out.z = sgd_elem(pv.z, gv.z, bv.z, o.neg_lr, o.mom, o.wd, o.first, b.z);
        out.w = sgd_elem(pv.w, gv.w, bv.w, o.neg_lr, o.mom, o.wd, o.first, b.w);
        if (use_buf) s1[i] = b;
    } else {
        float4 mv = in.m, vv = in.v;
#define FH_ADAM_LANE(c) out.c = adam_elem(pv.c, gv.c, mv.c, vv.c, o.wd, o.decay_mul, o.decoupled, \
                                          o.one_m_b1, o.b2, o.one_m_b2, bc2_sqrt, o.eps, neg_step)
        FH_ADAM_LANE(x); FH_ADAM_LANE(y); FH_ADAM_LANE(z); FH_ADAM_LANE(w);
#undef FH_ADAM_LANE
        s1[i] = mv;
        s2[i] = vv;
    }
    p[i] = out;
}

// The same two phases for one element (a lane of the linear WGRAD tile owns single floats of
// 16 rows): opt_apply4's operations on one lane, element for element.
struct OptIn1 {
    float p, m, v;
};
template <bool ADAM>
__device__ __forceinline__ void opt_load1(const float* p, const float* s1, const float* s2,
                                          int64_t i, OptIn1& in) {
    in.p = p[i];
    in.m = (s1 ? s1 : p)[i];
    if constexpr (ADAM) in.v = s2[i];
}

template <bool ADAM>
__device__ __forceinline__ void opt_apply1(float* p, float* s1, float* s2, int64_t i,
                                           const OptIn1& in, float gv, const OptScal& o,
                                           float bc2_sqrt, float neg_step) {
    float out;
    if constexpr (!ADAM) {
        const bool use_buf = o.mom != 0.f;
        const float bv = (use_buf && !o.first) ? in.m : 0.f;
        float b;
        out = sgd_elem(in.p, gv, bv, o.neg_lr, o.mom, o.wd, o.first, b);
        if (use_buf) s1[i] = b;
    } else {
        float mv = in.m, vv = in.v;
        out = adam_elem(in.p, gv, mv, vv, o.wd, o.decay_mul, o.decoupled, o.one_m_b1, o.b2,
                        o.one_m_b2, bc2_sqrt, o.eps, neg_step);
        s1[i] = mv;
        s2[i] = vv;
    }
    p[i] = out;
}

}  // namespace fh
