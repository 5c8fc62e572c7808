// rsx_sac.hip — gradients of the soft actor-critic losses of include/rsx.h (rsx_task_sac_gradient) with respect to an MLP actor with a
// squashed Gaussian head (rsx_gaussian_head.hpp), one or two MLP critics on [obs | action] and the log-temperature.  Six launches, no
// state of an env is read or written; a translation unit of its own so that the instantiations of every existing kernel stay exactly
// what they were.  The scheme and the device pieces are rsx_dpg.hip's (rsx_qnet.hpp: one wave per workgroup, one row per lane, the weights
// as LDS broadcasts of the transposed image, the hidden layers' weight gradients on the f32 MFMA continuing ONE running partial per
// workgroup, a reduce in workgroup order).
//
// 1. sac_target_kernel<HA, HC>: forward only.  The actor and the C target critics lie in LDS side by side.  Lane r takes minibatch entry
//    t = block * 64 + r: a', logp' from the head on next_obs with the draw of position t under domain 12, the critics on [next_obs | a'],
//    y[t] and logp'[t] into the workspace.
// 2. sac_critic_kernel<H>: grid (G, C).  rsx_dpg.hip's critic launch: the squared-error head against y[t], weight gradients.
// 3. sac_sample_kernel<HA>: forward only, the actor alone: a~, logp from the head on obs with the draw under domain 13, into the workspace.
// 4. sac_qa_kernel<HC>: grid (G, C).  Critic c alone: Q_c(obs, a~) and, backward WITHOUT weight gradients down to its first layer's dz1,
//    dQ_c/da from the action rows of its first-layer image, into the workspace.
// 5. sac_actor_kernel<HA>: the actor alone, forward once more (the same bits), the selected critic's dQ/da and the entropy term through
//    tanh, the reparameterisation and the log-std clamp into all 2 AD output rows, then the backward pass with weight gradients.
// 6. sac_reduce_kernel: one thread per output element sums the partials in workgroup order from 0.0f; one more folds the stats.
// The actor and both critics never share a workgroup's LDS: the largest launch is the target launch (rsx_dpg.hip's plus the wider output
// layer).  The grid of the row launches is G = min(ceil(M / 64), max_workgroups): the bits depend on the inputs and that number alone.
#include <hip/hip_runtime.h>

#include "rsx.h"
#include "rsx_gaussian_head.hpp"
#include "rsx_launch.hpp"
#include "rsx_plan_common.hpp"
#include "rsx_policy_mlp.hpp"
#include "rsx_qnet.hpp"
#include "rsx_units.hpp"

namespace rsx {

namespace {

// the draws: counter (minibatch position, noise_step hi, noise_step lo, domain | block << 8); domain word 12 for next_obs, 13 for obs
// (rsx_math.hpp: 1, 3 .. 7; rsx_ppo_update.hip: 8; rsx_selfplay.hip: 9; rsx_dpg.hip: 10; rsx_dpg_update.hip: 11).  Named SAC_DRAW_*, not
// DOM_*: tests/test_dpg_update_build.py pins the set of DOM_* words as it stood with that unit; tests/test_sac_build.py pins the whole
// set, these two included, and that no word is taken twice
constexpr uint32_t SAC_DRAW_NEXT = 12u, SAC_DRAW_OBS = 13u;
enum : int { SAC_OUT_STATS = 12, SAC_DEFAULT_WORKGROUPS = 256, SAC_AP = 8 };   // SAC_AP: the pitch of the per-entry action arrays of the workspace
// the stats terms of a partial.  critic: 0 sum of (q - y)^2, 1 sum of q, 2 sum of y, 3 sum of logp', 4 entries used (int bits), 5 entries
// skipped (int bits).  actor: 0 sum of alpha * logp - min Q, 1 sum of logp, 2 sum of logp + target_entropy

struct SacArgs {
    Net actor, critic;           // the launch's own: the target critics for the target launch
    const float* obs;            // [N][OD]
    const float* action;         // [N][AD]
    const float* reward;         // [N]
    const float* next_obs;       // [N][OD]
    const uint8_t* terminated;   // [N]
    const int32_t* rows;         // [M] or nullptr
    const float* log_alpha;      // [1]
    float* y;                    // [M] workspace: the targets
    float* nlogp;                // [M] workspace: logp'
    float* logp;                 // [M] workspace: logp
    float* at;                   // [M][SAC_AP] workspace: a~
    float* qa;                   // [C][M4] workspace: Q_c(obs, a~)
    float* dqda;                 // [C][M][SAC_AP] workspace: dQ_c/da at (obs, a~)
    float* part;                 // the launch's partials [.][G][stride]
    float* out_target;           // [M] or nullptr
    float* out_q;                // [C][M] or nullptr
    float* out_action;           // [M][AD] or nullptr
    float* out_logp;             // [M] or nullptr
    float* out_nlogp;            // [M] or nullptr
    float* out_eps;              // [M][AD] or nullptr
    float* out_neps;             // [M][AD] or nullptr
    float* out_mean;             // [M][AD] or nullptr
    float* out_ls;               // [M][AD] or nullptr
    const long long* step_dev;   // nullptr: step
    long long step;
    long long N, M, M4;
    uint32_t k0, k1;
    int stride, OD, AD, C;
    int wide, wide_next;         // OD % 4 == 0 and the array 16-byte aligned: rows are read four floats at a time
    float gamma, target_entropy, ls_min, ls_max, inv_m;
    const float* discount;       // [N] or nullptr: the row's own discount in place of gamma (rsx_grad_per)
    const float* weight;         // [M] or nullptr: the entry's weight on the critic loss
};

// LDS of the row kernels, in floats
struct SacTargetLds { int critic, A, total; };
__host__ __device__ inline SacTargetLds sac_target_lds(const PolicyImage& ma, const PolicyImage& mc, const int HA, const int HC, const int C) {
    SacTargetLds t;
    t.critic = ma.rows;                       // C images behind the actor's
    t.A = t.critic + C * mc.rows;             // [64][max(HA, HC) + 4]
    t.total = t.A + 64 * (max_i(HA, HC) + 4);
    return t;
}
struct SacCriticLds { int A, D, O, idx, total; };
__host__ __device__ inline SacCriticLds sac_critic_lds(const PolicyImage& mc, const int HC) {
    SacCriticLds c;
    c.A = mc.rows;
    c.D = c.A + 64 * (HC + 4);
    c.O = c.D + 64 * 33;
    c.idx = c.O + 64;
    c.total = c.idx + 64;
    return c;
}
struct SacQaLds { int A, O, total; };
__host__ __device__ inline SacQaLds sac_qa_lds(const PolicyImage& mc, const int HC) {
    SacQaLds c;
    c.A = mc.rows;                            // [64][HC + 4]: h1, then dz1
    c.O = c.A + 64 * (HC + 4);                // [64]: dQ/dQ
    c.total = c.O + 64;
    return c;
}
struct SacActorLds { int A, D, O, idx, total; };
__host__ __device__ inline SacActorLds sac_actor_lds(const PolicyImage& ma, const int HA, const int AD) {
    SacActorLds a;
    a.A = ma.rows;                            // [64][HA + 4]: h1, then dz1; the final stats fold
    a.D = a.A + 64 * (HA + 4);                // [64][33]
    a.O = a.D + 64 * 33;                      // [64][(2 AD) | 1]: dL/dmu, dL/draw
    a.idx = a.O + 64 * ((2 * AD) | 1);
    a.total = a.idx + 64;
    return a;
}

// lane's entry of block blk (rsx_dpg.hip's gather): its position t, whether it lies in the minibatch and in the batch, and the row it reads
struct SacEntry { long long t, idx; bool in_m, live; };
__device__ __forceinline__ SacEntry sac_gather(const SacArgs& G, const long long blk, const int lane) {
    SacEntry e;
    e.t = blk * 64 + lane;
    e.in_m = e.t < G.M;
    e.idx = 0;
    if (e.in_m) e.idx = G.rows != nullptr ? (long long)G.rows[e.t] : e.t;
    e.live = e.in_m && e.idx >= 0 && e.idx < G.N;
    if (!e.live) e.idx = 0;   // (a row that exists; everything it contributes is selected away)
    return e;
}

struct SacStep { uint32_t lo, hi; };
__device__ __forceinline__ SacStep sac_step(const SacArgs& G) {
    const long long step = G.step_dev != nullptr ? *G.step_dev : G.step;
    return SacStep{(uint32_t)((unsigned long long)step & 0xFFFFFFFFull), (uint32_t)((unsigned long long)step >> 32)};
}
// the AD standard normals of minibatch position t under domain word dom: component k takes normal k & 3 of block k >> 2 (the collector's recipe)
__device__ __forceinline__ void sac_eps(const SacArgs& G, const long long t, const SacStep st, const uint32_t dom, float (&eps)[DPG_MAX_ACT]) {
    u32x4 u{};
#pragma unroll
    for (int k = 0; k < DPG_MAX_ACT; ++k) {
        eps[k] = 0.0f;
        if (k < G.AD) {
            if ((k & 3) == 0) u = philox4x32((uint32_t)t, st.hi, st.lo, dom | ((uint32_t)(k >> 2) << 8), G.k0, G.k1);
            float n0, n1;
            plan_normal_pair((k & 2) ? u.z : u.x, (k & 2) ? u.w : u.y, n0, n1);
            eps[k] = (k & 1) ? n1 : n0;
        }
    }
}

template <int HA, int HC>
__global__ __launch_bounds__(64) void sac_target_kernel(const SacArgs G) {
    extern __shared__ float4 sac_lds4[];
    float* const lds = reinterpret_cast<float*>(sac_lds4);
    const int lane = threadIdx.x;
    const int OD = G.OD, AD = G.AD;
    const PolicyImage ma = gaussian_image(0, OD, AD, G.actor.layers, HA);
    const PolicyImage mc = policy_image(0, OD + AD, 1, G.critic.layers, HC);
    const SacTargetLds L = sac_target_lds(ma, mc, HA, HC, G.C);
    stage_policy(G.actor.params, lds, ma, stage_args(G.actor, HA), OD, 2 * AD, lane);
    for (int c = 0; c < G.C; ++c)
        stage_policy(G.critic.params + (size_t)c * (size_t)G.critic.n_params, lds + L.critic + c * mc.rows, mc, stage_args(G.critic, HC),
                     OD + AD, 1, lane);
    float* const A = lds + L.A;
    const SacStep st = sac_step(G);
    const float alpha = exp_f32(*G.log_alpha);
    wave_sync();
#pragma nounroll
    for (long long blk = blockIdx.x; blk * 64 < G.M; blk += gridDim.x) {
        const SacEntry e = sac_gather(G, blk, lane);
        const float* __restrict__ x = G.next_obs + (size_t)e.idx * (size_t)OD;
        float ap[DPG_MAX_ACT], eps[DPG_MAX_ACT];
        float logp = 0.0f;
        sac_eps(G, e.t, st, SAC_DRAW_NEXT, eps);
        {
            float none[DPG_MAX_ACT];
#pragma unroll
            for (int k = 0; k < DPG_MAX_ACT; ++k) none[k] = 0.0f;
            float h[HA];
            forward_hidden<HA>(lds, ma, G.actor.layers, G.actor.hidden_act, x, OD, G.wide_next, none, 0, A + lane * (HA + 4), h);
#pragma unroll
            for (int k = 0; k < DPG_MAX_ACT; ++k) {
                ap[k] = 0.0f;
                if (k < AD) {
                    const HeadOut o = squashed_head(output_unit<HA>(lds, ma, k, h), output_unit<HA>(lds, ma, AD + k, h), eps[k], G.ls_min, G.ls_max);
                    ap[k] = o.a;
                    logp = k == 0 ? o.term : logp + o.term;
                    if (G.out_neps != nullptr && e.in_m) G.out_neps[(size_t)e.t * (size_t)AD + k] = e.live ? eps[k] : 0.0f;
                }
            }
        }
        float qmin = 0.0f;
        for (int c = 0; c < G.C; ++c) {
            float h[HC];
            const float* img = lds + L.critic + c * mc.rows;
            forward_hidden<HC>(img, mc, G.critic.layers, G.critic.hidden_act, x, OD, G.wide_next, ap, AD, A + lane * (HC + 4), h);
            const float q = output_unit<HC>(img, mc, 0, h);
            qmin = c == 0 ? q : fminf(qmin, q);
        }
        if (e.in_m) {
            const float r = G.reward[e.idx];
            const float gm = G.discount != nullptr ? G.discount[e.idx] : G.gamma;
            const float y = G.terminated[e.idx] != 0 ? r : r + gm * (qmin - alpha * logp);
            G.y[e.t] = e.live ? y : 0.0f;
            G.nlogp[e.t] = e.live ? logp : 0.0f;
            if (G.out_target != nullptr) G.out_target[e.t] = e.live ? y : 0.0f;
            if (G.out_nlogp != nullptr) G.out_nlogp[e.t] = e.live ? logp : 0.0f;
        }
    }
}

template <int H>
__global__ __launch_bounds__(64) void sac_critic_kernel(const SacArgs G) {
    extern __shared__ float4 sac_lds4[];
    float* const lds = reinterpret_cast<float*>(sac_lds4);
    const int lane = threadIdx.x;
    const int OD = G.OD, AD = G.AD, c = blockIdx.y, kind = G.critic.hidden_act, layers = G.critic.layers;
    const PolicyImage m = policy_image(0, OD + AD, 1, layers, H);
    const SacCriticLds L = sac_critic_lds(m, H);
    stage_policy(G.critic.params + (size_t)c * (size_t)G.critic.n_params, lds, m, stage_args(G.critic, H), OD + AD, 1, lane);
    float* const A = lds + L.A;
    float* const D = lds + L.D;
    float* const O = lds + L.O;
    int* const idxs = reinterpret_cast<int*>(lds + L.idx);
    wave_sync();
    float* const part = G.part + ((size_t)c * gridDim.x + blockIdx.x) * (size_t)G.stride;
    const InputRows X{G.obs, G.action, OD, AD};
    float st0 = 0.0f, st1 = 0.0f, st2 = 0.0f, st3 = 0.0f;
    int used = 0, skipped = 0;
    bool first = true;
#pragma nounroll
    for (long long blk = blockIdx.x; blk * 64 < G.M; blk += gridDim.x, first = false) {
        const SacEntry e = sac_gather(G, blk, lane);
        used += e.live ? 1 : 0;
        skipped += (e.in_m && !e.live) ? 1 : 0;
        idxs[lane] = (int)e.idx;
        float ext[DPG_MAX_ACT];
#pragma unroll
        for (int k = 0; k < DPG_MAX_ACT; ++k) ext[k] = k < AD ? G.action[(size_t)e.idx * (size_t)AD + k] : 0.0f;
        float h[H];
        forward_hidden<H>(lds, m, layers, kind, G.obs + (size_t)e.idx * (size_t)OD, OD, G.wide, ext, AD, A + lane * (H + 4), h);
        const float q = output_unit<H>(lds, m, 0, h);
        if (G.out_q != nullptr && e.in_m) G.out_q[(size_t)c * (size_t)G.M + (size_t)e.t] = e.live ? q : 0.0f;
        const float y = e.in_m ? G.y[e.t] : 0.0f;
        const float diff = q - y;
        const float w = G.weight != nullptr && e.in_m ? G.weight[e.t] : 1.0f;   // (times 1.0f is exact: the plain call's bits)
        O[lane] = e.live ? (diff * w) * G.inv_m : 0.0f;
        if (e.live) {
            st0 += (w * diff) * diff;
            st1 += q;
            st2 += y;
            st3 += G.nlogp[e.t];
        }
        backward<H, true>(lds, m, layers, kind, A, D, O, 1, 1, h, e.live, first, lane, part, X, idxs);
    }
    fold_stats(A, part + G.critic.n_params, lane, st0, st1, st2, st3, used, skipped);
}

template <int HA>
__global__ __launch_bounds__(64) void sac_sample_kernel(const SacArgs G) {
    extern __shared__ float4 sac_lds4[];
    float* const lds = reinterpret_cast<float*>(sac_lds4);
    const int lane = threadIdx.x;
    const int OD = G.OD, AD = G.AD;
    const PolicyImage ma = gaussian_image(0, OD, AD, G.actor.layers, HA);
    stage_policy(G.actor.params, lds, ma, stage_args(G.actor, HA), OD, 2 * AD, lane);
    float* const A = lds + ma.rows;   // [64][HA + 4]
    const SacStep st = sac_step(G);
    wave_sync();
#pragma nounroll
    for (long long blk = blockIdx.x; blk * 64 < G.M; blk += gridDim.x) {
        const SacEntry e = sac_gather(G, blk, lane);
        float none[DPG_MAX_ACT], eps[DPG_MAX_ACT];
#pragma unroll
        for (int k = 0; k < DPG_MAX_ACT; ++k) none[k] = 0.0f;
        sac_eps(G, e.t, st, SAC_DRAW_OBS, eps);
        float h[HA];
        forward_hidden<HA>(lds, ma, G.actor.layers, G.actor.hidden_act, G.obs + (size_t)e.idx * (size_t)OD, OD, G.wide, none, 0,
                           A + lane * (HA + 4), h);
        float logp = 0.0f;
#pragma unroll
        for (int k = 0; k < DPG_MAX_ACT; ++k) {
            if (k < AD) {
                const float mu = output_unit<HA>(lds, ma, k, h), raw = output_unit<HA>(lds, ma, AD + k, h);
                const HeadOut o = squashed_head(mu, raw, eps[k], G.ls_min, G.ls_max);
                logp = k == 0 ? o.term : logp + o.term;
                if (e.in_m) {
                    const size_t at = (size_t)e.t * (size_t)AD + k;
                    G.at[(size_t)e.t * SAC_AP + k] = e.live ? o.a : 0.0f;
                    if (G.out_action != nullptr) G.out_action[at] = e.live ? o.a : 0.0f;
                    if (G.out_eps != nullptr) G.out_eps[at] = e.live ? eps[k] : 0.0f;
                    if (G.out_mean != nullptr) G.out_mean[at] = e.live ? mu : 0.0f;
                    if (G.out_ls != nullptr) G.out_ls[at] = e.live ? o.ls : 0.0f;
                }
            }
        }
        if (e.in_m) {
            G.logp[e.t] = e.live ? logp : 0.0f;
            if (G.out_logp != nullptr) G.out_logp[e.t] = e.live ? logp : 0.0f;
        }
    }
}

template <int HC>
__global__ __launch_bounds__(64) void sac_qa_kernel(const SacArgs G) {
    extern __shared__ float4 sac_lds4[];
    float* const lds = reinterpret_cast<float*>(sac_lds4);
    const int lane = threadIdx.x;
    const int OD = G.OD, AD = G.AD, c = blockIdx.y, kind = G.critic.hidden_act, layers = G.critic.layers;
    const PolicyImage mc = policy_image(0, OD + AD, 1, layers, HC);
    const SacQaLds L = sac_qa_lds(mc, HC);
    stage_policy(G.critic.params + (size_t)c * (size_t)G.critic.n_params, lds, mc, stage_args(G.critic, HC), OD + AD, 1, lane);
    float* const Ac = lds + L.A;
    float* const Oc = lds + L.O;
    wave_sync();
    const InputRows Xc{G.obs, nullptr, OD, AD};
#pragma nounroll
    for (long long blk = blockIdx.x; blk * 64 < G.M; blk += gridDim.x) {
        const SacEntry e = sac_gather(G, blk, lane);
        float at[DPG_MAX_ACT];
#pragma unroll
        for (int k = 0; k < DPG_MAX_ACT; ++k) at[k] = (k < AD && e.in_m) ? G.at[(size_t)e.t * SAC_AP + k] : 0.0f;
        float h[HC];
        forward_hidden<HC>(lds, mc, layers, kind, G.obs + (size_t)e.idx * (size_t)OD, OD, G.wide, at, AD, Ac + lane * (HC + 4), h);
        const float q = output_unit<HC>(lds, mc, 0, h);
        if (e.in_m) G.qa[(size_t)c * (size_t)G.M4 + (size_t)e.t] = e.live ? q : 0.0f;
        Oc[lane] = e.live ? 1.0f : 0.0f;   // dQ/dQ: the sign and the 1 / M are the actor launch's
        backward<HC, false>(lds, mc, layers, kind, Ac, nullptr, Oc, 1, 1, h, e.live, true, lane, nullptr, Xc, nullptr);
        // ---- dQ/da_k = sum over j of W1[j][OD + k] * dz1[j] (four interleaved chains, (s0 + s1) + (s2 + s3)) ----
#pragma unroll
        for (int k = 0; k < DPG_MAX_ACT; ++k) {
            if (k < AD) {
                const float* wrow = lds + mc.w1 + (OD + k) * (HC + 4);
                const float* dz = Ac + lane * (HC + 4);
                float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
                for (int q4 = 0; q4 < HC / 4; ++q4) {
                    const float4 w = reinterpret_cast<const float4*>(wrow)[q4];
                    const float4 d = reinterpret_cast<const float4*>(dz)[q4];
                    s0 = fma_(w.x, d.x, s0);
                    s1 = fma_(w.y, d.y, s1);
                    s2 = fma_(w.z, d.z, s2);
                    s3 = fma_(w.w, d.w, s3);
                }
                if (e.in_m) G.dqda[((size_t)c * (size_t)G.M + (size_t)e.t) * SAC_AP + k] = e.live ? (s0 + s1) + (s2 + s3) : 0.0f;
            }
        }
        wave_sync();   // Ac and Oc are read: the next trip may overwrite them
    }
}

template <int HA>
__global__ __launch_bounds__(64) void sac_actor_kernel(const SacArgs G) {
    extern __shared__ float4 sac_lds4[];
    float* const lds = reinterpret_cast<float*>(sac_lds4);
    const int lane = threadIdx.x;
    const int OD = G.OD, AD = G.AD, OP = (2 * AD) | 1;
    const PolicyImage ma = gaussian_image(0, OD, AD, G.actor.layers, HA);
    const SacActorLds L = sac_actor_lds(ma, HA, AD);
    stage_policy(G.actor.params, lds, ma, stage_args(G.actor, HA), OD, 2 * AD, lane);
    float* const Aa = lds + L.A;
    float* const D = lds + L.D;
    float* const Oa = lds + L.O;
    int* const idxs = reinterpret_cast<int*>(lds + L.idx);
    const SacStep st = sac_step(G);
    const float alpha = exp_f32(*G.log_alpha);
    wave_sync();
    float* const part = G.part + (size_t)blockIdx.x * (size_t)G.stride;
    const InputRows Xa{G.obs, nullptr, OD, 0};
    float st0 = 0.0f, st1 = 0.0f, st2 = 0.0f;
    bool first = true;
#pragma nounroll
    for (long long blk = blockIdx.x; blk * 64 < G.M; blk += gridDim.x, first = false) {
        const SacEntry e = sac_gather(G, blk, lane);
        idxs[lane] = (int)e.idx;
        float none[DPG_MAX_ACT], eps[DPG_MAX_ACT];
#pragma unroll
        for (int k = 0; k < DPG_MAX_ACT; ++k) none[k] = 0.0f;
        sac_eps(G, e.t, st, SAC_DRAW_OBS, eps);
        float h[HA];
        forward_hidden<HA>(lds, ma, G.actor.layers, G.actor.hidden_act, G.obs + (size_t)e.idx * (size_t)OD, OD, G.wide, none, 0,
                           Aa + lane * (HA + 4), h);
        // the critic that gives the minimum passes its dQ/da; on an exact tie critic 0 passes
        const float q0 = e.in_m ? G.qa[e.t] : 0.0f;
        const float q1 = (e.in_m && G.C == 2) ? G.qa[(size_t)G.M4 + (size_t)e.t] : q0;
        const int sel = q1 < q0 ? 1 : 0;
        const float qmin = sel ? q1 : q0;
        float logp = 0.0f;
#pragma unroll
        for (int k = 0; k < DPG_MAX_ACT; ++k) {
            if (k < AD) {
                const float mu = output_unit<HA>(lds, ma, k, h), raw = output_unit<HA>(lds, ma, AD + k, h);
                const HeadOut o = squashed_head(mu, raw, eps[k], G.ls_min, G.ls_max);
                logp = k == 0 ? o.term : logp + o.term;
                const float dq = e.in_m ? G.dqda[((size_t)sel * (size_t)G.M + (size_t)e.t) * SAC_AP + k] : 0.0f;
                // d(alpha logp - Q)/du = alpha * 2 a - dQ/da * (1 - a^2), with 1 - a^2 = fmaf(-a, a, 1); eps is a constant
                const float du = (alpha * (2.0f * o.a) - dq * fma_(-o.a, o.a, 1.0f)) * G.inv_m;
                // ... /dls = du * sigma * eps - alpha (logp's own -ls term), through the clamp as torch.clamp: bounds included
                const float dls = du * (o.sigma * eps[k]) - alpha * G.inv_m;
                const bool inside = raw >= G.ls_min && raw <= G.ls_max;
                Oa[lane * OP + k] = e.live ? du : 0.0f;
                Oa[lane * OP + AD + k] = (e.live && inside) ? dls : 0.0f;
            }
        }
        if (e.live) {
            st0 += alpha * logp - qmin;
            st1 += logp;
            st2 += logp + G.target_entropy;
        }
        backward<HA, true>(lds, ma, G.actor.layers, G.actor.hidden_act, Aa, D, Oa, OP, 2 * AD, h, e.live, first, lane, part, Xa, idxs);
    }
    fold_stats(Aa, part + G.actor.n_params, lane, st0, st1, st2, 0.0f, 0, 0);
}

struct SacReduceArgs {
    const float* part_c;   // [C][grid][stride_c]
    const float* part_a;   // [grid][stride_a]
    const float* log_alpha;
    float* grad_c;         // [C][Pc]
    float* grad_a;         // [Pa]
    float* grad_log_alpha; // [1]
    float* stats;          // [SAC_OUT_STATS]
    int grid, stride_c, stride_a, Pc, Pa, C;
    float inv_m;
};

__global__ __launch_bounds__(256) void sac_reduce_kernel(const SacReduceArgs R) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int n_c = R.C * R.Pc, n = n_c + R.Pa;
    if (e < n_c) {
        const int c = e / R.Pc, k = e - c * R.Pc;
        R.grad_c[e] = sum_partials(R.part_c + (size_t)c * R.grid * R.stride_c + k, R.grid, R.stride_c);
    } else if (e < n) {
        R.grad_a[e - n_c] = sum_partials(R.part_a + (e - n_c), R.grid, R.stride_a);
    } else if (e == n) {
        const float* s0 = R.part_c + R.Pc;
        const float* sa = R.part_a + R.Pa;
        for (int c = 0; c < 2; ++c) {
            const float* sc = s0 + (size_t)c * R.grid * R.stride_c;
            R.stats[c] = c < R.C ? (0.5f * sum_partials(sc + 0, R.grid, R.stride_c)) * R.inv_m : 0.0f;
            R.stats[2 + c] = c < R.C ? sum_partials(sc + 1, R.grid, R.stride_c) * R.inv_m : 0.0f;
        }
        const float log_alpha = *R.log_alpha;
        const float excess = sum_partials(sa + 2, R.grid, R.stride_a) * R.inv_m;   // mean(logp + target_entropy)
        R.stats[4] = sum_partials(sa + 0, R.grid, R.stride_a) * R.inv_m;
        R.stats[5] = -(log_alpha * excess);
        R.stats[6] = sum_partials(s0 + 2, R.grid, R.stride_c) * R.inv_m;
        R.stats[7] = sum_partials(sa + 1, R.grid, R.stride_a) * R.inv_m;
        R.stats[8] = sum_partials(s0 + 3, R.grid, R.stride_c) * R.inv_m;
        R.stats[9] = exp_f32(log_alpha);
        R.stats[10] = (float)sum_partials_int(s0 + 4, R.grid, R.stride_c);
        R.stats[11] = (float)sum_partials_int(s0 + 5, R.grid, R.stride_c);
        R.grad_log_alpha[0] = -excess;
    }
}

template <int ID, typename K>
void sac_launch_rows(K kernel, const dim3 grid, const size_t lds, hipStream_t s, const SacArgs& G) {
    grant_lds<ID>((const void*)kernel, lds);
    rsx_launch(kernel, grid, dim3(64), lds, s, G);
}

int sac_stride_of(const long long n_params) { return (int)(n_params + DPG_PART_STATS); }

}  // namespace

int sac_grid(const long long n_rows, const int max_workgroups) {
    const long long trips = (n_rows + 63) / 64;
    const long long cap = max_workgroups > 0 ? max_workgroups : (int)SAC_DEFAULT_WORKGROUPS;
    return (int)(trips < cap ? trips : cap);
}

long long sac_lds_bytes(const int launch, const int obs_dim, const int act_dim, const PolicySpec& actor, const PolicySpec& critic,
                        const int n_critics) {
    const PolicyImage ma = gaussian_image(0, obs_dim, act_dim, actor.layers, actor.hidden);
    const PolicyImage mc = policy_image(0, obs_dim + act_dim, 1, critic.layers, critic.hidden);
    const int floats = launch == SAC_LAUNCH_TARGET   ? sac_target_lds(ma, mc, actor.hidden, critic.hidden, n_critics).total
                       : launch == SAC_LAUNCH_CRITIC ? sac_critic_lds(mc, critic.hidden).total
                       : launch == SAC_LAUNCH_SAMPLE ? ma.rows + 64 * (actor.hidden + 4)
                       : launch == SAC_LAUNCH_QA     ? sac_qa_lds(mc, critic.hidden).total
                                                     : sac_actor_lds(ma, actor.hidden, act_dim).total;
    return (long long)sizeof(float) * floats;
}

// y, logp', logp [M4] each; a~ [M][8]; Q_c(obs, a~) [C][M4]; dQ_c/da [C][M][8]; one partial per workgroup and network
long long sac_workspace_bytes(const long long n_params_actor, const long long n_params_critic, const int n_critics, const long long n_rows,
                              const int max_workgroups) {
    const long long grid = sac_grid(n_rows, max_workgroups), m4 = round4ll(n_rows);
    return (long long)sizeof(float) * ((3 + n_critics) * m4 + (1 + n_critics) * n_rows * SAC_AP +
                                       grid * ((long long)n_critics * sac_stride_of(n_params_critic) + sac_stride_of(n_params_actor)));
}

void launch_sac_gradient(const PolicySpec& actor, const long long n_params_actor, const float* actor_params, const PolicySpec& critic,
                         const long long n_params_critic, const float* critic_params, const float* target_critic_params,
                         const float* log_alpha, const int obs_dim, const int act_dim, const rsx_dpg_in& in, const rsx_sac_cfg& cfg,
                         const rsx_sac_out& out, hipStream_t s, const rsx_grad_per* per) {
    const int C = cfg.n_critics;
    const int grid = sac_grid(in.n_rows, cfg.max_workgroups);
    const int stride_c = sac_stride_of(n_params_critic), stride_a = sac_stride_of(n_params_actor);
    const long long M = in.n_rows, M4 = round4ll(M);
    float* const y = static_cast<float*>(out.workspace);
    float* const nlogp = y + M4;
    float* const logp = nlogp + M4;
    float* const at = logp + M4;
    float* const qa = at + M * SAC_AP;
    float* const dqda = qa + C * M4;
    float* const part_c = dqda + (size_t)C * (size_t)M * SAC_AP;
    float* const part_a = part_c + (size_t)C * (size_t)grid * (size_t)stride_c;
    const float inv_m = 1.0f / (float)in.n_rows;
    const auto wide = [&](const float* p) { return (int)(obs_dim % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0); };
    SacArgs G{};
    G.obs = in.obs; G.action = in.action; G.reward = in.reward; G.next_obs = in.next_obs; G.terminated = in.terminated; G.rows = in.rows;
    G.log_alpha = log_alpha;
    if (per != nullptr) { G.discount = per->discount; G.weight = per->weight; }
    G.y = y; G.nlogp = nlogp; G.logp = logp; G.at = at; G.qa = qa; G.dqda = dqda;
    G.out_target = out.target; G.out_q = out.q; G.out_action = out.action; G.out_logp = out.log_prob; G.out_nlogp = out.next_log_prob;
    G.out_eps = out.eps; G.out_neps = out.next_eps; G.out_mean = out.mean; G.out_ls = out.log_std;
    G.step_dev = reinterpret_cast<const long long*>(cfg.noise_step_dev); G.step = (long long)cfg.noise_step;
    G.N = in.n_batch_rows; G.M = M; G.M4 = M4;
    G.k0 = (uint32_t)(cfg.noise_seed & 0xFFFFFFFFull); G.k1 = (uint32_t)(cfg.noise_seed >> 32);
    G.OD = obs_dim; G.AD = act_dim; G.C = C;
    G.wide = wide(in.obs); G.wide_next = wide(in.next_obs);
    G.gamma = cfg.gamma; G.target_entropy = cfg.target_entropy; G.ls_min = cfg.log_std_min; G.ls_max = cfg.log_std_max; G.inv_m = inv_m;
    const Net net_a{actor_params, (int)n_params_actor, actor.layers, actor.hidden_act, actor.out_act};
    const Net net_c{critic_params, (int)n_params_critic, critic.layers, critic.hidden_act, critic.out_act};
    const int ha = actor.hidden, hc = critic.hidden;
    const auto lds_of = [&](const int launch) { return (size_t)sac_lds_bytes(launch, obs_dim, act_dim, actor, critic, C); };
    const dim3 g1((unsigned)grid), gc((unsigned)grid, (unsigned)C);
    // (1) the targets: the actor with the target critics
    G.actor = net_a; G.critic = net_c; G.critic.params = target_critic_params;
    if (ha == 64 && hc == 64) sac_launch_rows<0>(sac_target_kernel<64, 64>, g1, lds_of(SAC_LAUNCH_TARGET), s, G);
    else if (ha == 64) sac_launch_rows<1>(sac_target_kernel<64, 32>, g1, lds_of(SAC_LAUNCH_TARGET), s, G);
    else if (hc == 64) sac_launch_rows<2>(sac_target_kernel<32, 64>, g1, lds_of(SAC_LAUNCH_TARGET), s, G);
    else sac_launch_rows<3>(sac_target_kernel<32, 32>, g1, lds_of(SAC_LAUNCH_TARGET), s, G);
    // (2) the critics
    G.critic = net_c;
    G.part = part_c; G.stride = stride_c;
    if (hc == 64) sac_launch_rows<4>(sac_critic_kernel<64>, gc, lds_of(SAC_LAUNCH_CRITIC), s, G);
    else sac_launch_rows<5>(sac_critic_kernel<32>, gc, lds_of(SAC_LAUNCH_CRITIC), s, G);
    // (3) a~ and logp
    if (ha == 64) sac_launch_rows<6>(sac_sample_kernel<64>, g1, lds_of(SAC_LAUNCH_SAMPLE), s, G);
    else sac_launch_rows<7>(sac_sample_kernel<32>, g1, lds_of(SAC_LAUNCH_SAMPLE), s, G);
    // (4) each critic on (obs, a~) and its dQ/da
    if (hc == 64) sac_launch_rows<8>(sac_qa_kernel<64>, gc, lds_of(SAC_LAUNCH_QA), s, G);
    else sac_launch_rows<9>(sac_qa_kernel<32>, gc, lds_of(SAC_LAUNCH_QA), s, G);
    // (5) the actor's backward pass
    G.part = part_a; G.stride = stride_a;
    if (ha == 64) sac_launch_rows<10>(sac_actor_kernel<64>, g1, lds_of(SAC_LAUNCH_ACTOR), s, G);
    else sac_launch_rows<11>(sac_actor_kernel<32>, g1, lds_of(SAC_LAUNCH_ACTOR), s, G);
    // (6) the reduce
    const SacReduceArgs R{part_c, part_a, log_alpha, out.grad_critics, out.grad_actor, out.grad_log_alpha, out.stats, grid, stride_c, stride_a,
                          (int)n_params_critic, (int)n_params_actor, C, inv_m};
    const int n = C * (int)n_params_critic + (int)n_params_actor + 1;
    rsx_launch(sac_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, R);
}

}  // namespace rsx
