// rsx_policy_mlp.hpp — the MLP policy of include/rsx.h (rsx_policy_mlp) as the kernels evaluate it: what rsx_policy.hip (the closed-loop
// lookahead) and rsx_collect.hip (on-policy collection) share.  One workgroup holds ONE policy:
//   weights     staged in LDS once per launch, TRANSPOSED ([input][unit], row pitch hidden + 4 floats): lane b of an env computes
//               the hidden / L consecutive units b * U .. b * U + U - 1 and reads their weights for input i as one or two 16-byte
//               reads; the L lanes of an env read disjoint slices of one row (no bank is hit twice), lanes with equal b in
//               different envs read the same address (a broadcast).  The pitch of hidden + 4 only serves the staging stores
//               (lanes walk i: pitch 64 would put all of them on one bank).
//   rows        the observation of an env is produced piecewise by its lanes (write_obs): it is assembled in an LDS row per env,
//               and every lane of the env reads it back four floats at a time; the hidden vectors travel the same way.  Row pitch:
//               a multiple of 4 floats whose quarter is odd, so the G = 64 / L rows start on different banks.
//   arithmetic  one lane computes a whole unit: acc = bias; for i ascending: acc = fmaf(W[j][i], x[i], acc), in float32.  No
//               cross-lane reduction, so the bits depend neither on L nor on the physics form.
// No MFMA: a wave holds 64 / L envs, i.e. at most eight columns of activations against a 64 x 64 matrix — the matrices are too thin,
// and an MFMA accumulates in an order of its own, which the fixed order above forbids (examples/fused_policy.hip says the same of
// its 10 MFLOP).
#pragma once
#include <hip/hip_runtime.h>

#include "rsx.h"
#include "rsx_math.hpp"

namespace rsx {

namespace {   // (kernel argument types and device code of kernels with internal linkage: one copy per unit, as the kernels themselves)

// ---- the LDS image of one policy: offsets in floats, every one a multiple of 4 ----
struct PolicyImage {
    int ws, as, xs;                    // row pitch of the hidden layers' weights, of the output layer's, of the per-env rows
    int w1, b1, w2, b2, wo, bo, rows;  // offsets; rows: [3][G][xs], then the actions [G][8]
    int total;                         // floats
};
__host__ __device__ inline int round4(const int n) { return (n + 3) & ~3; }
__host__ __device__ inline PolicyImage policy_image(const int G, const int OD, const int AD, const int layers, const int H) {
    PolicyImage m;
    m.ws = H + 4;
    m.as = AD | 1;
    const int n4 = round4(OD > H ? OD : H);
    m.xs = ((n4 >> 2) & 1) ? n4 : n4 + 4;
    m.w1 = 0;
    m.b1 = m.w1 + OD * m.ws;
    m.w2 = m.b1 + H;
    m.b2 = m.w2 + (layers == 2 ? H * m.ws : 0);
    m.wo = m.b2 + (layers == 2 ? H : 0);
    m.bo = m.wo + round4(H * m.as);
    m.rows = m.bo + 8;
    m.total = m.rows + 3 * G * m.xs + G * 8;
    return m;
}

struct PolicyArgs {
    const float* params;   // [n_policies][P]
    const float* obs;      // the handle's obs buffer [num_envs][obs_dim] (read only)
    float* actions_out;    // [num_envs][K][H][act_dim] or nullptr
    float* obs_out;        // [num_envs][K][H][obs_dim] or nullptr
    int n_params;          // P
    int layers, hidden, hidden_act, out_act;
};

// tanh in float32 with a fixed operation order (the unit is built with -ffp-contract=off): the odd Cephes polynomial below 0.625,
// 1 - 2 / (exp(2 |x|) + 1) above, on the hardware's exp2 and reciprocal (1 ulp each).  |result| <= 1: e >= 1, so 2 / (e + 1) is in [0, 1].
__device__ __forceinline__ float tanh_f32(const float x) {
    const float ax = fabsf(x), z = x * x;
    const float p = fma_(fma_(fma_(fma_(fma_(-5.70498872745e-3f, z, 2.06390887954e-2f), z, -5.37397155531e-2f), z, 1.33314422036e-1f), z,
                              -3.33332819422e-1f) * z, x, x);
    const float e = __builtin_amdgcn_exp2f(ax * 2.8853900817779268f);
    const float r = 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
    return ax < 0.625f ? p : __builtin_copysignf(r, x);
}

__device__ __forceinline__ float policy_act(const float v, const int kind) {
    switch (kind) {
        case RSX_ACT_RELU: return fmaxf(v, 0.0f);
        case RSX_ACT_CLIP: return clampf(v, -1.0f, 1.0f);
        default: return tanh_f32(v);
    }
}

// U consecutive floats from a 4 * U-byte aligned LDS address
template <int U>
__device__ __forceinline__ void load_units(const float* p, float (&w)[U]) {
    if constexpr (U >= 4) {
#pragma unroll
        for (int q = 0; q < U / 4; ++q) {
            const float4 v = reinterpret_cast<const float4*>(p)[q];
            w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
        }
    } else if constexpr (U == 2) {
        const float2 v = *reinterpret_cast<const float2*>(p);
        w[0] = v.x; w[1] = v.y;
    } else {
        w[0] = p[0];
    }
}

// one hidden layer: this lane's U = H / L units of its env.  wt: [n_in][H + 4] transposed weights, x: the env's input row
template <int H, int L>
__device__ __forceinline__ void hidden_layer(const float* wt, const float* bias, const float* x, const int n_in, const int b, const int act,
                                             float* out) {
    constexpr int U = H / L, WS = H + 4;
    float acc[U], w[U];
    load_units<U>(bias + b * U, acc);
    const float* wl = wt + b * U;
    int i = 0;
#pragma nounroll   // (one block of four inputs in flight: unrolled over a constant obs_dim the weight reads took every register)
    for (; i + 4 <= n_in; i += 4) {
        const float4 xv = *reinterpret_cast<const float4*>(x + i);
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            load_units<U>(wl + (i + c) * WS, w);
#pragma unroll
            for (int u = 0; u < U; ++u) acc[u] = fma_(w[u], xs[c], acc[u]);
        }
    }
#pragma nounroll
    for (; i < n_in; ++i) {
        const float xi = x[i];
        load_units<U>(wl + i * WS, w);
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = fma_(w[u], xi, acc[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) out[b * U + u] = policy_act(acc[u], act);
}

// rows [j][n_in] of a torch.nn.Linear weight -> LDS [i][pitch] (+ j); the bias behind it -> LDS
__device__ __forceinline__ void stage_layer(const float* __restrict__ w, const int n_out, const int n_in, float* wt, const int pitch,
                                            float* bias, const int lane) {
#pragma unroll 4
    for (int j = 0; j < n_out; ++j)
        for (int i = lane; i < n_in; i += 64) wt[i * pitch + j] = w[(size_t)j * n_in + i];
    for (int j = lane; j < n_out; j += 64) bias[j] = w[(size_t)n_out * n_in + j];
}

// the policy's answer to the rows in xo: the action of lane b < AD's component in oa[g][b] (the caller synchronises).  OUT_ACT = false
// (the collector's stochastic head): the output layer's accumulator as it stands, the activation is the caller's
template <int H, int L, int AD, bool OUT_ACT = true>
__device__ __forceinline__ float policy_forward(float* lds, const PolicyImage& m, const PolicyArgs& Q, const int OD, const int b, const int g) {
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
    float acc = 0.0f;
    if (b < AD) {
        const float* wo = lds + m.wo + b;
        acc = lds[m.bo + b];
#pragma unroll 2
        for (int i = 0; i < H; i += 4) {
            const float4 hv = *reinterpret_cast<const float4*>(h + i);
            acc = fma_(wo[i * m.as], hv.x, acc);
            acc = fma_(wo[(i + 1) * m.as], hv.y, acc);
            acc = fma_(wo[(i + 2) * m.as], hv.z, acc);
            acc = fma_(wo[(i + 3) * m.as], hv.w, acc);
        }
        if constexpr (OUT_ACT) acc = policy_act(acc, Q.out_act);
    }
    return acc;
}

// the weights of policy `w` ([P], rsx.h's layout) -> the image, by all 64 lanes of the workgroup (the caller synchronises)
__device__ __forceinline__ void stage_policy(const float* __restrict__ w, float* lds, const PolicyImage& m, const PolicyArgs& Q, const int OD,
                                             const int AD, const int lane) {
    const int H = Q.hidden;
    stage_layer(w, H, OD, lds + m.w1, m.ws, lds + m.b1, lane);
    w += (size_t)H * OD + H;
    if (Q.layers == 2) {
        stage_layer(w, H, H, lds + m.w2, m.ws, lds + m.b2, lane);
        w += (size_t)H * H + H;
    }
    stage_layer(w, AD, H, lds + m.wo, m.as, lds + m.bo, lane);
}

}  // namespace

}  // namespace rsx
