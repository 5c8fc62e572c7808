// rsx_gaussian_head.hpp — the squashed Gaussian head of include/rsx.h (rsx_task_collect_gaussian) as the kernels evaluate it, next to
// rsx_policy_mlp.hpp, whose pieces it builds on and restates none of: the state-dependent head's LDS image (rsx_policy_mlp.hpp's with an
// output layer of 2 * act_dim units), its forward (the hidden layers are hidden_layer's; lane b < AD computes output unit b, the mean, AND
// unit AD + b, the raw log-std, so both land in the lane that squashes component b: no cross-lane exchange, and AD <= L stays the only
// lane condition), and exp in float32 with a fixed operation order.
#pragma once
#include <hip/hip_runtime.h>

#include "rsx.h"
#include "rsx_math.hpp"
#include "rsx_policy_mlp.hpp"

namespace rsx {

namespace {

// exp in float32 with a fixed operation order (the unit is built with -ffp-contract=off), on the hardware's exp2 (1 ulp), the way tanh_f32
// is.  The product x * log2(e) is taken in two floats (the fmaf recovers the rounding error of the head, the tail constant carries what
// float32 drops of log2 e), so that the error of the exponent does not grow with |x|: exp(x) = exp2(t) * (1 + r ln 2), |r| < 2^-18.
// Relative error below 5e-7 for x in [-80, 80] (include/rsx.h states the bound; tests/test_gpu_sac.py measures it).
__device__ __forceinline__ float exp_f32(const float x) {
    const float t = x * 1.44269502162933349609375f;                            // the float32 head of log2(e)
    const float r = fma_(x, 1.925963033500011e-8f, fma_(x, 1.44269502162933349609375f, -t));   // + its tail: log2(e) - head
    const float e = __builtin_amdgcn_exp2f(t);
    return fma_(e, r * 0.693147182464599609375f, e);
}

// log1p on [0, 1] in float32 with a fixed operation order, on the hardware's log2 and reciprocal (1 ulp each): w = 1 + y rounds, d = w - 1
// is exact, and log(w) * (y / d) puts back what the rounding of w took (d == 0: y itself).  Absolute error below 3e-7 on [0, 1].
__device__ __forceinline__ float log1p_f32(const float y) {
    const float w = 1.0f + y;
    const float d = w - 1.0f;
    const float l = __builtin_amdgcn_logf(w) * 0.693147182464599609375f;
    const float c = y * __builtin_amdgcn_rcpf(d);
    return d == 0.0f ? y : l * c;
}

// the squashed head of include/rsx.h for one component, every operation rounded in the order written: the clamped log-std, sigma, the
// pre-tanh sample u, the action a and the component's term of the log-probability, the tanh correction in its stable form
// 2 (ln 2 - u - softplus(-2 u)), softplus(z) = max(z, 0) + log1p(exp(-|z|))
struct HeadOut { float ls, sigma, u, a, term; };
__device__ __forceinline__ HeadOut squashed_head(const float mu, const float raw, const float eps, const float lo, const float hi) {
    HeadOut o;
    o.ls = clampf(raw, lo, hi);
    o.sigma = exp_f32(o.ls);
    o.u = mu + o.sigma * eps;   // (two roundings)
    o.a = tanh_f32(o.u);
    const float z = -2.0f * o.u;
    const float sp = fmaxf(z, 0.0f) + log1p_f32(exp_f32(-fabsf(z)));
    const float g = ((-0.5f * eps) * eps - o.ls) - 0.918938517570495605469f;   // 0.5 ln(2 pi)
    o.term = g - 2.0f * ((0.693147182464599609375f - o.u) - sp);
    return o;
}

// the image of a policy whose output layer is 2 * AD wide: policy_image's offsets up to the output layer, then that layer at pitch
// (2 AD) | 1 with a bias slot of 16 floats, the rows and the action slots behind it.  policy_image itself returns what it returned.
__host__ __device__ inline PolicyImage gaussian_image(const int G, const int OD, const int AD, const int layers, const int H) {
    PolicyImage m = policy_image(G, OD, AD, layers, H);
    m.as = (2 * AD) | 1;
    m.bo = m.wo + round4(H * m.as);
    m.rows = m.bo + 16;
    m.total = m.rows + 3 * G * m.xs + G * 8;
    return m;
}

// the head's answer to the row of env g: mu (the return value) and raw (the log-std before the clamp) of component b < AD, both the
// output layer's accumulator as it stands: acc = bias; for i ascending: acc = fmaf(W[j][i], h[i], acc) — rsx_policy_mlp.hpp's arithmetic,
// so mu and raw are the bits every other evaluation of the same parameters on the same observation gives.  The caller synchronises.
template <int H, int L, int AD>
__device__ __forceinline__ float gaussian_forward(float* lds, const PolicyImage& m, const PolicyArgs& Q, const int OD, const int b, const int g,
                                                  float& raw) {
    constexpr int G = 64 / L;
    const float* xo = lds + m.rows + g * m.xs;
    float* ha = lds + m.rows + (G + g) * m.xs;
    float* hb = lds + m.rows + (2 * G + g) * m.xs;
    hidden_layer<H, L>(lds + m.w1, lds + m.b1, xo, OD, b, Q.hidden_act, ha);
    wave_sync();
    const float* h = ha;
    if (Q.layers == 2) {
        hidden_layer<H, L>(lds + m.w2, lds + m.b2, ha, H, b, Q.hidden_act, hb);
        wave_sync();
        h = hb;
    }
    float mu = 0.0f;
    raw = 0.0f;
    if (b < AD) {
        const float* wm = lds + m.wo + b;
        const float* wr = wm + AD;
        mu = lds[m.bo + b];
        raw = lds[m.bo + AD + b];
#pragma unroll 2
        for (int i = 0; i < H; i += 4) {   // two independent chains, each ascending in i
            const float4 hv = *reinterpret_cast<const float4*>(h + i);
            mu = fma_(wm[i * m.as], hv.x, mu);             raw = fma_(wr[i * m.as], hv.x, raw);
            mu = fma_(wm[(i + 1) * m.as], hv.y, mu);       raw = fma_(wr[(i + 1) * m.as], hv.y, raw);
            mu = fma_(wm[(i + 2) * m.as], hv.z, mu);       raw = fma_(wr[(i + 2) * m.as], hv.z, raw);
            mu = fma_(wm[(i + 3) * m.as], hv.w, mu);       raw = fma_(wr[(i + 3) * m.as], hv.w, raw);
        }
    }
    return mu;
}

}  // namespace

}  // namespace rsx
