// rsx_dpg.hip — gradients of the deterministic-policy-gradient losses of include/rsx.h (rsx_task_dpg_gradient: TD3 with two critics and
// target smoothing, DDPG with one critic and none) with respect to an MLP actor and one or two MLP critics whose input row is
// [obs | action].  Four launches, no state of an env is read or written; a translation unit of its own so that the instantiations of
// every existing kernel stay exactly what they were.  The scheme is rsx_ppo.hip's (one wave per workgroup, one row per lane, the
// weights as LDS broadcasts of the transposed image, the hidden layers' weight gradients on the f32 MFMA continuing ONE running partial
// per workgroup, a reduce in workgroup order); the device pieces live in rsx_qnet.hpp, which rsx_sac.hip includes too.
//
// 1. dpg_target_kernel<HA, HC>: forward only.  The target actor and the C target critics lie in LDS side by side.  Lane r takes
//    minibatch entry t = block * 64 + r: a' from the target actor on next_obs and the smoothing noise of position t, the critics on
//    [next_obs | a'], y[t] and sum |a'| into the workspace.
// 2. dpg_critic_kernel<H>: grid (G, C).  rsx_ppo.hip's row kernel with the squared-error head against y[t]; the first layer's input
//    and the B operand of its weight gradient come from two arrays (columns below obs_dim from obs, the rest from action).
// 3. dpg_actor_kernel<HA, HC>: the actor and critic 0 lie in LDS side by side.  Forward the actor, forward critic 0 on [obs | pi(obs)],
//    backward critic 0 WITHOUT weight gradients down to its first layer's dz1, dQ/da from the action rows of its first-layer image,
//    through out_act, then the actor's backward pass with weight gradients.  Skipped when no actor gradient is asked for.
// 4. dpg_reduce_kernel: one thread per output element sums the partials in workgroup order from 0.0f; one more thread folds the stats.
// The grid of the row launches is G = min(ceil(M / 64), max_workgroups): the bits depend on the inputs and that number alone.
#include <hip/hip_runtime.h>

#include "rsx.h"
#include "rsx_launch.hpp"
#include "rsx_plan_common.hpp"
#include "rsx_policy_mlp.hpp"
#include "rsx_qnet.hpp"
#include "rsx_units.hpp"

namespace rsx {

namespace {

constexpr uint32_t DOM_DPG = 10u;   // the smoothing noise: counter (minibatch position, noise_step hi, noise_step lo, DPG | block << 8)
enum : int { DPG_OUT_STATS = 9, DPG_DEFAULT_WORKGROUPS = 256 };
// (one workgroup per CU by LDS for the target and the actor launch on 256 CUs; a constant, not the device's)
// the stats terms of a partial.  critic: 0 sum of (q - y)^2, 1 sum of q, 2 sum of y, 3 sum of sum_k |a'_k|, 4 entries used (int bits),
// 5 entries skipped (int bits).  actor: 0 sum of Q_0(obs, pi(obs))

struct DpgArgs {
    Net actor, critic;           // the launch's own: the target networks for the target launch
    const float* obs;            // [N][OD]
    const float* action;         // [N][AD]
    const float* reward;         // [N]
    const float* next_obs;       // [N][OD]
    const uint8_t* terminated;   // [N]
    const int32_t* rows;         // [M] or nullptr
    float* y;                    // [M] workspace: the targets
    float* absa;                 // [M] workspace: sum over k of |a'_k|
    float* part;                 // the launch's partials [.][G][stride]
    float* out_target;           // [M] or nullptr
    float* out_q;                // [C][M] or nullptr
    float* out_action;           // [M][AD] or nullptr
    float* out_noise;            // [M][AD] or nullptr
    const long long* step_dev;   // nullptr: step
    long long step;
    long long N, M;
    uint32_t k0, k1;
    int stride, OD, AD, C;
    int wide, wide_next;         // OD % 4 == 0 and the array 16-byte aligned: rows are read four floats at a time
    float gamma, sigma, noise_clip, inv_m;
    const float* discount;       // [N] or nullptr: the row's own discount in place of gamma (rsx_grad_per)
    const float* weight;         // [M] or nullptr: the entry's weight on the critic loss
};

// LDS of the three row kernels, in floats
struct TargetLds { int actor, critic, A, total; };
__host__ __device__ inline TargetLds target_lds(const PolicyImage& ma, const PolicyImage& mc, const int HA, const int HC, const int C) {
    TargetLds t;
    t.actor = 0;
    t.critic = ma.rows;                       // C images
    t.A = t.critic + C * mc.rows;             // [64][max(HA, HC) + 4]
    t.total = t.A + 64 * (max_i(HA, HC) + 4);
    return t;
}
struct CriticLds { int A, D, O, idx, total; };
__host__ __device__ inline CriticLds critic_lds(const PolicyImage& mc, const int HC) {
    CriticLds c;
    c.A = mc.rows;
    c.D = c.A + 64 * (HC + 4);
    c.O = c.D + 64 * 33;
    c.idx = c.O + 64;
    c.total = c.idx + 64;
    return c;
}
struct ActorLds { int critic, Aa, Ta, Ac, D, Oa, Oc, idx, total; };
__host__ __device__ inline ActorLds actor_lds(const PolicyImage& ma, const PolicyImage& mc, const int HA, const int HC, const int AD) {
    ActorLds a;
    a.critic = ma.rows;
    a.Aa = a.critic + mc.rows;                // [64][HA + 4]: the actor's h1, then its dz1
    a.Ta = a.Aa + 64 * (HA + 4);              // [64][HA + 4]: the actor's top activations while critic 0 runs
    a.Ac = a.Ta + 64 * (HA + 4);              // [64][HC + 4]: critic 0's h1, then its dz1; the final stats fold
    a.D = a.Ac + 64 * (HC + 4);               // [64][33]
    a.Oa = a.D + 64 * 33;                     // [64][AD | 1]: the mean, then dL/dmean
    a.Oc = a.Oa + 64 * (AD | 1);              // [64]: dL/dQ
    a.idx = a.Oc + 64;
    a.total = a.idx + 64;
    return a;
}

// lane's entry of block blk: its position t, whether it lies in the minibatch and in the batch, and the row it reads (0 when dead)
struct Entry { long long t, idx; bool in_m, live; };
__device__ __forceinline__ Entry gather(const DpgArgs& G, const long long blk, const int lane) {
    Entry e;
    e.t = blk * 64 + lane;
    e.in_m = e.t < G.M;
    e.idx = 0;
    if (e.in_m) e.idx = G.rows != nullptr ? (long long)G.rows[e.t] : e.t;
    e.live = e.in_m && e.idx >= 0 && e.idx < G.N;
    if (!e.live) e.idx = 0;   // (a row that exists; everything it contributes is selected away)
    return e;
}

template <int HA, int HC>
__global__ __launch_bounds__(64) void dpg_target_kernel(const DpgArgs G) {
    extern __shared__ float4 dpg_lds4[];
    float* const lds = reinterpret_cast<float*>(dpg_lds4);
    const int lane = threadIdx.x;
    const int OD = G.OD, AD = G.AD;
    const PolicyImage ma = policy_image(0, OD, AD, G.actor.layers, HA);
    const PolicyImage mc = policy_image(0, OD + AD, 1, G.critic.layers, HC);
    const TargetLds L = target_lds(ma, mc, HA, HC, G.C);
    stage_policy(G.actor.params, lds + L.actor, ma, stage_args(G.actor, HA), OD, AD, lane);
    for (int c = 0; c < G.C; ++c)
        stage_policy(G.critic.params + (size_t)c * (size_t)G.critic.n_params, lds + L.critic + c * mc.rows, mc, stage_args(G.critic, HC),
                     OD + AD, 1, lane);
    float* const A = lds + L.A;
    const bool noisy = G.sigma != 0.0f;
    const long long step = G.step_dev != nullptr ? *G.step_dev : G.step;
    const uint32_t step_lo = (uint32_t)((unsigned long long)step & 0xFFFFFFFFull), step_hi = (uint32_t)((unsigned long long)step >> 32);
    wave_sync();
#pragma nounroll
    for (long long blk = blockIdx.x; blk * 64 < G.M; blk += gridDim.x) {
        const Entry e = gather(G, blk, lane);
        const float* __restrict__ x = G.next_obs + (size_t)e.idx * (size_t)OD;
        float ap[DPG_MAX_ACT];
        float absa = 0.0f;
        {
            float none[DPG_MAX_ACT];
#pragma unroll
            for (int k = 0; k < DPG_MAX_ACT; ++k) none[k] = 0.0f;
            float h[HA];
            forward_hidden<HA>(lds + L.actor, ma, G.actor.layers, G.actor.hidden_act, x, OD, G.wide_next, none, 0, A + lane * (HA + 4), h);
            u32x4 u{};
#pragma unroll
            for (int k = 0; k < DPG_MAX_ACT; ++k) {
                ap[k] = 0.0f;
                if (k < AD) {
                    float a = policy_act(output_unit<HA>(lds + L.actor, ma, k, h), G.actor.out_act);
                    float nz = 0.0f;
                    if (noisy) {
                        // component k takes normal k & 3 of block k >> 2 (the collector's recipe)
                        if ((k & 3) == 0) u = philox4x32((uint32_t)e.t, step_hi, step_lo, DOM_DPG | ((uint32_t)(k >> 2) << 8), G.k0, G.k1);
                        float n0, n1;
                        plan_normal_pair((k & 2) ? u.z : u.x, (k & 2) ? u.w : u.y, n0, n1);
                        nz = clampf(G.sigma * ((k & 1) ? n1 : n0), -G.noise_clip, G.noise_clip);
                        a = clampf(a + nz, -1.0f, 1.0f);
                    }
                    ap[k] = a;
                    absa = k == 0 ? fabsf(a) : absa + fabsf(a);
                    if (G.out_noise != nullptr && e.in_m) G.out_noise[(size_t)e.t * (size_t)AD + k] = e.live ? nz : 0.0f;
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
            const float y = G.terminated[e.idx] != 0 ? r : r + gm * qmin;
            G.y[e.t] = e.live ? y : 0.0f;
            G.absa[e.t] = e.live ? absa : 0.0f;
            if (G.out_target != nullptr) G.out_target[e.t] = e.live ? y : 0.0f;
        }
    }
}

template <int H>
__global__ __launch_bounds__(64) void dpg_critic_kernel(const DpgArgs G) {
    extern __shared__ float4 dpg_lds4[];
    float* const lds = reinterpret_cast<float*>(dpg_lds4);
    const int lane = threadIdx.x;
    const int OD = G.OD, AD = G.AD, c = blockIdx.y, kind = G.critic.hidden_act, layers = G.critic.layers;
    const PolicyImage m = policy_image(0, OD + AD, 1, layers, H);
    const CriticLds L = critic_lds(m, H);
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
        const Entry e = gather(G, blk, lane);
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
            st3 += G.absa[e.t];
        }
        backward<H, true>(lds, m, layers, kind, A, D, O, 1, 1, h, e.live, first, lane, part, X, idxs);
    }
    fold_stats(A, part + G.critic.n_params, lane, st0, st1, st2, st3, used, skipped);
}

template <int HA, int HC>
__global__ __launch_bounds__(64) void dpg_actor_kernel(const DpgArgs G) {
    extern __shared__ float4 dpg_lds4[];
    float* const lds = reinterpret_cast<float*>(dpg_lds4);
    const int lane = threadIdx.x;
    const int OD = G.OD, AD = G.AD, OP = AD | 1;
    const PolicyImage ma = policy_image(0, OD, AD, G.actor.layers, HA);
    const PolicyImage mc = policy_image(0, OD + AD, 1, G.critic.layers, HC);
    const ActorLds L = actor_lds(ma, mc, HA, HC, AD);
    stage_policy(G.actor.params, lds, ma, stage_args(G.actor, HA), OD, AD, lane);
    stage_policy(G.critic.params, lds + L.critic, mc, stage_args(G.critic, HC), OD + AD, 1, lane);   // (critic 0)
    const float* const imgc = lds + L.critic;
    float* const Aa = lds + L.Aa;
    float* const Ta = lds + L.Ta;
    float* const Ac = lds + L.Ac;
    float* const D = lds + L.D;
    float* const Oa = lds + L.Oa;
    float* const Oc = lds + L.Oc;
    int* const idxs = reinterpret_cast<int*>(lds + L.idx);
    wave_sync();
    float* const part = G.part + (size_t)blockIdx.x * (size_t)G.stride;
    const InputRows Xa{G.obs, nullptr, OD, 0}, Xc{G.obs, nullptr, OD, AD};
    float st0 = 0.0f;
    bool first = true;
#pragma nounroll
    for (long long blk = blockIdx.x; blk * 64 < G.M; blk += gridDim.x, first = false) {
        const Entry e = gather(G, blk, lane);
        idxs[lane] = (int)e.idx;
        const float* __restrict__ x = G.obs + (size_t)e.idx * (size_t)OD;
        float pi[DPG_MAX_ACT];
        {
            float none[DPG_MAX_ACT];
#pragma unroll
            for (int k = 0; k < DPG_MAX_ACT; ++k) none[k] = 0.0f;
            float h[HA];
            forward_hidden<HA>(lds, ma, G.actor.layers, G.actor.hidden_act, x, OD, G.wide, none, 0, Aa + lane * (HA + 4), h);
#pragma unroll
            for (int k = 0; k < DPG_MAX_ACT; ++k) {
                pi[k] = 0.0f;
                if (k < AD) {
                    const float mean = output_unit<HA>(lds, ma, k, h);
                    Oa[lane * OP + k] = mean;
                    pi[k] = policy_act(mean, G.actor.out_act);
                    if (G.out_action != nullptr && e.in_m) G.out_action[(size_t)e.t * (size_t)AD + k] = e.live ? pi[k] : 0.0f;
                }
            }
            store_vec<HA>(Ta + lane * (HA + 4), h);
        }
        {
            // ---- critic 0 on [obs | pi(obs)], and back to its first layer's dz1 (in Ac) ----
            float h[HC];
            forward_hidden<HC>(imgc, mc, G.critic.layers, G.critic.hidden_act, x, OD, G.wide, pi, AD, Ac + lane * (HC + 4), h);
            const float q = output_unit<HC>(imgc, mc, 0, h);
            if (e.live) st0 += q;
            Oc[lane] = e.live ? -G.inv_m : 0.0f;   // dL_pi / dQ
            backward<HC, false>(imgc, mc, G.critic.layers, G.critic.hidden_act, Ac, D, Oc, 1, 1, h, e.live, first, lane, nullptr, Xc, idxs);
        }
        // ---- dL/da_k = sum over j of W1[j][OD + k] * dz1[j] (four interleaved chains, (s0 + s1) + (s2 + s3)), then through out_act ----
#pragma unroll
        for (int k = 0; k < DPG_MAX_ACT; ++k) {
            if (k < AD) {
                const float* wrow = imgc + mc.w1 + (OD + k) * (HC + 4);
                const float* dz = Ac + lane * (HC + 4);
                float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
                for (int q = 0; q < HC / 4; ++q) {
                    const float4 w = reinterpret_cast<const float4*>(wrow)[q];
                    const float4 d = reinterpret_cast<const float4*>(dz)[q];
                    s0 = fma_(w.x, d.x, s0);
                    s1 = fma_(w.y, d.y, s1);
                    s2 = fma_(w.z, d.z, s2);
                    s3 = fma_(w.w, d.w, s3);
                }
                const float da = (s0 + s1) + (s2 + s3);
                const float mean = Oa[lane * OP + k];
                const float dact = G.actor.out_act == RSX_ACT_TANH ? fma_(-pi[k], pi[k], 1.0f) : ((mean >= -1.0f && mean <= 1.0f) ? 1.0f : 0.0f);
                Oa[lane * OP + k] = e.live ? da * dact : 0.0f;
            }
        }
        {
            float h[HA];
            load_vec<HA>(Ta + lane * (HA + 4), h);
            backward<HA, true>(lds, ma, G.actor.layers, G.actor.hidden_act, Aa, D, Oa, OP, AD, h, e.live, first, lane, part, Xa, idxs);
        }
    }
    fold_stats(Ac, part + G.actor.n_params, lane, st0, 0.0f, 0.0f, 0.0f, 0, 0);
}

struct ReduceArgs {
    const float* part_c;   // [C][grid][stride_c]
    const float* part_a;   // [grid][stride_a] or nullptr
    float* grad_c;         // [C][Pc]
    float* grad_a;         // [Pa] or nullptr
    float* stats;          // [DPG_OUT_STATS]
    int grid, stride_c, stride_a, Pc, Pa, C, AD;
    float inv_m;
};

__global__ __launch_bounds__(256) void dpg_reduce_kernel(const ReduceArgs R) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int n_c = R.C * R.Pc, n = n_c + (R.part_a != nullptr ? R.Pa : 0);
    if (e < n_c) {
        const int c = e / R.Pc, k = e - c * R.Pc;
        R.grad_c[e] = sum_partials(R.part_c + (size_t)c * R.grid * R.stride_c + k, R.grid, R.stride_c);
    } else if (e < n) {
        R.grad_a[e - n_c] = sum_partials(R.part_a + (e - n_c), R.grid, R.stride_a);
    } else if (e == n) {
        const float* s0 = R.part_c + R.Pc;
        for (int c = 0; c < 2; ++c) {
            const float* sc = s0 + (size_t)c * R.grid * R.stride_c;
            R.stats[c] = c < R.C ? (0.5f * sum_partials(sc + 0, R.grid, R.stride_c)) * R.inv_m : 0.0f;
            R.stats[2 + c] = c < R.C ? sum_partials(sc + 1, R.grid, R.stride_c) * R.inv_m : 0.0f;
        }
        R.stats[4] = R.part_a != nullptr ? -(sum_partials(R.part_a + R.Pa, R.grid, R.stride_a) * R.inv_m) : 0.0f;
        R.stats[5] = sum_partials(s0 + 2, R.grid, R.stride_c) * R.inv_m;
        R.stats[6] = (sum_partials(s0 + 3, R.grid, R.stride_c) * R.inv_m) / (float)R.AD;
        R.stats[7] = (float)sum_partials_int(s0 + 4, R.grid, R.stride_c);
        R.stats[8] = (float)sum_partials_int(s0 + 5, R.grid, R.stride_c);
    }
}

template <int ID, typename K>
void launch_rows(K kernel, const dim3 grid, const size_t lds, hipStream_t s, const DpgArgs& G) {
    grant_lds<ID>((const void*)kernel, lds);
    rsx_launch(kernel, grid, dim3(64), lds, s, G);
}

int stride_of(const long long n_params) { return (int)(n_params + DPG_PART_STATS); }

}  // namespace

int dpg_grid(const long long n_rows, const int max_workgroups) {
    const long long trips = (n_rows + 63) / 64;
    const long long cap = max_workgroups > 0 ? max_workgroups : (int)DPG_DEFAULT_WORKGROUPS;
    return (int)(trips < cap ? trips : cap);
}

long long dpg_lds_bytes(const int launch, const int obs_dim, const int act_dim, const PolicySpec& actor, const PolicySpec& critic,
                        const int n_critics) {
    const PolicyImage ma = policy_image(0, obs_dim, act_dim, actor.layers, actor.hidden);
    const PolicyImage mc = policy_image(0, obs_dim + act_dim, 1, critic.layers, critic.hidden);
    const int floats = launch == DPG_LAUNCH_TARGET   ? target_lds(ma, mc, actor.hidden, critic.hidden, n_critics).total
                       : launch == DPG_LAUNCH_CRITIC ? critic_lds(mc, critic.hidden).total
                                                     : actor_lds(ma, mc, actor.hidden, critic.hidden, act_dim).total;
    return (long long)sizeof(float) * floats;
}

long long dpg_workspace_bytes(const long long n_params_actor, const long long n_params_critic, const int n_critics, const long long n_rows,
                              const int max_workgroups) {
    const long long grid = dpg_grid(n_rows, max_workgroups);
    return (long long)sizeof(float) * (2 * round4ll(n_rows) + grid * ((long long)n_critics * stride_of(n_params_critic) + stride_of(n_params_actor)));
}

void launch_dpg_gradient(const PolicySpec& actor, const long long n_params_actor, const float* actor_params, const float* target_actor_params,
                         const PolicySpec& critic, const long long n_params_critic, const float* critic_params,
                         const float* target_critic_params, const int obs_dim, const int act_dim, const rsx_dpg_in& in, const rsx_dpg_cfg& cfg,
                         const rsx_dpg_out& out, hipStream_t s, const rsx_grad_per* per) {
    const int C = cfg.n_critics;
    const int grid = dpg_grid(in.n_rows, cfg.max_workgroups);
    const int stride_c = stride_of(n_params_critic), stride_a = stride_of(n_params_actor);
    float* const y = static_cast<float*>(out.workspace);
    float* const absa = y + round4ll(in.n_rows);
    float* const part_c = absa + round4ll(in.n_rows);
    float* const part_a = part_c + (size_t)C * (size_t)grid * (size_t)stride_c;
    const float inv_m = 1.0f / (float)in.n_rows;
    const auto wide = [&](const float* p) { return (int)(obs_dim % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0); };
    DpgArgs G{};
    G.obs = in.obs; G.action = in.action; G.reward = in.reward; G.next_obs = in.next_obs; G.terminated = in.terminated; G.rows = in.rows;
    G.y = y; G.absa = absa;
    G.out_target = out.target; G.out_q = out.q; G.out_action = out.action; G.out_noise = out.target_noise;
    G.step_dev = reinterpret_cast<const long long*>(cfg.noise_step_dev); G.step = (long long)cfg.noise_step;
    G.N = in.n_batch_rows; G.M = in.n_rows;
    G.k0 = (uint32_t)(cfg.noise_seed & 0xFFFFFFFFull); G.k1 = (uint32_t)(cfg.noise_seed >> 32);
    G.OD = obs_dim; G.AD = act_dim; G.C = C;
    G.wide = wide(in.obs); G.wide_next = wide(in.next_obs);
    G.gamma = cfg.gamma; G.sigma = cfg.sigma; G.noise_clip = cfg.noise_clip; G.inv_m = inv_m;
    if (per != nullptr) { G.discount = per->discount; G.weight = per->weight; }
    const Net net_a{actor_params, (int)n_params_actor, actor.layers, actor.hidden_act, actor.out_act};
    const Net net_c{critic_params, (int)n_params_critic, critic.layers, critic.hidden_act, critic.out_act};
    const int ha = actor.hidden, hc = critic.hidden;
    // (a) the targets
    G.actor = net_a; G.actor.params = target_actor_params;
    G.critic = net_c; G.critic.params = target_critic_params;
    {
        const size_t lds = (size_t)dpg_lds_bytes(DPG_LAUNCH_TARGET, obs_dim, act_dim, actor, critic, C);
        const dim3 g((unsigned)grid);
        if (ha == 64 && hc == 64) launch_rows<0>(dpg_target_kernel<64, 64>, g, lds, s, G);
        else if (ha == 64) launch_rows<1>(dpg_target_kernel<64, 32>, g, lds, s, G);
        else if (hc == 64) launch_rows<2>(dpg_target_kernel<32, 64>, g, lds, s, G);
        else launch_rows<3>(dpg_target_kernel<32, 32>, g, lds, s, G);
    }
    // (b) the critics
    G.actor = net_a; G.critic = net_c;
    G.part = part_c; G.stride = stride_c;
    {
        const size_t lds = (size_t)dpg_lds_bytes(DPG_LAUNCH_CRITIC, obs_dim, act_dim, actor, critic, C);
        const dim3 g((unsigned)grid, (unsigned)C);
        if (hc == 64) launch_rows<4>(dpg_critic_kernel<64>, g, lds, s, G);
        else launch_rows<5>(dpg_critic_kernel<32>, g, lds, s, G);
    }
    // (c) the actor through critic 0
    const bool with_actor = out.grad_actor != nullptr;
    if (with_actor) {
        G.part = part_a; G.stride = stride_a;
        const size_t lds = (size_t)dpg_lds_bytes(DPG_LAUNCH_ACTOR, obs_dim, act_dim, actor, critic, C);
        const dim3 g((unsigned)grid);
        if (ha == 64 && hc == 64) launch_rows<6>(dpg_actor_kernel<64, 64>, g, lds, s, G);
        else if (ha == 64) launch_rows<7>(dpg_actor_kernel<64, 32>, g, lds, s, G);
        else if (hc == 64) launch_rows<8>(dpg_actor_kernel<32, 64>, g, lds, s, G);
        else launch_rows<9>(dpg_actor_kernel<32, 32>, g, lds, s, G);
    }
    // (d) the reduce
    const ReduceArgs R{part_c, with_actor ? part_a : nullptr, out.grad_critics, out.grad_actor, out.stats, grid, stride_c, stride_a,
                       (int)n_params_critic, (int)n_params_actor, C, act_dim, inv_m};
    const int n = C * (int)n_params_critic + (with_actor ? (int)n_params_actor : 0) + 1;
    rsx_launch(dpg_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, R);
}

}  // namespace rsx
