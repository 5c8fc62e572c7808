// rsx_collect_gaussian.hip — collection under a state-dependent, tanh-squashed Gaussian head (soft actor-critic's actor): the handle's
// envs advanced n steps under an MLP whose output layer gives mean AND log-std per state, inside ONE launch, with auto-reset, and the
// [T][B] batch written out (include/rsx.h: rsx_task_collect_gaussian).  A translation unit of its own so that the instantiations of
// every existing kernel stay exactly what they were: rsx_collect.hip says why its loop is not a hook in the shared body, and the same
// holds for a hook in rsx_collect.hip's loop.
//
// task_collect_gaussian_kernel follows the loop of task_collect_policy_kernel piece by piece (the same step pieces and text fragments, so
// the handle ends up bit for bit where n rsx_task_step calls with the recorded actions leave it) with another action source:
//   mu_k, raw_k = the two output units k and AD + k (rsx_gaussian_head.hpp: gaussian_forward, rsx_policy_mlp.hpp's arithmetic)
//   ls_k = clamp(raw_k, log_std_min, log_std_max);  sigma_k = exp_f32(ls_k);  u_k = mu_k + sigma_k * eps_k (two roundings)
//   a_k = tanh_f32(u_k)                              deterministic: u_k = mu_k, no draw
// eps is the collector's own draw (domain word 7, the same counter and key).  log-probabilities are not computed here: the caller has
// mean, log_std and sample.
//
// Grid: the handle's lane-group grid (lane_grid), one 64-lane workgroup per tile.  LDS: gaussian_image plus Shared<L> (VSS-v0 3v3 with
// 2 x 64 units: 36 928 B of image next to rsx_collect.hip's 36 384 B, 43 200 B with Shared<8> — three workgroups per CU, as there).
//
// Memory traffic of the loop: stores only, as in rsx_collect.hip: every load is issued ahead of the loop and lands behind ONE vmcnt(0).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rsx.h"
#include "rsx_gaussian_head.hpp"
#include "rsx_plan_common.hpp"
#include "rsx_policy_mlp.hpp"
#include "rsx_units.hpp"
#include "rsx_variants.hpp"

namespace rsx {

namespace {

struct GaussianArgs {
    float* obs;            // [T][B][obs_dim]
    float* actions;        // [T][B][act_dim]
    float* rewards;        // [T][B]
    uint8_t* flags;        // [T][B] bit 0 terminated, bit 1 truncated
    float* final_obs;      // [T][B][obs_dim] or nullptr: rows of ended (t, env) only
    float* mean;           // [T][B][act_dim] or nullptr
    float* sample;         // [T][B][act_dim] or nullptr
    float* log_std;        // [T][B][act_dim] or nullptr: the clamped log-std
    float ls_min, ls_max;
    int deterministic;
    uint32_t k0, k1;       // noise_seed lo, hi: the Philox key of the head's noise
};

template <int KIND, int TASK, int L, int NR, bool PHYS>
__global__ __launch_bounds__(64) void task_collect_gaussian_kernel(const float* __restrict__ params, float* __restrict__ obs_out,
                                                                   float* __restrict__ act_out, const int per_xcd, const int n_steps_arg,
                                                                   const Params P, const Buffers bufs, const PolicyArgs Q, const GaussianArgs C,
                                                                   float* phys) {
    using K = KC<KIND>;
    using T = TC<TASK>;
    constexpr int G = 64 / L;
    constexpr int ID = T::info_dim;
    constexpr int AD = T::act_dim;
    constexpr int MODE = MODE_ROLLOUT;   // (what the shared fragments specialise on: the multi-step trip)
    constexpr int mode = 0;
    static_assert(TASK != RSX_TASK_SSL_SCRIMMAGE && AD <= 8 && AD <= L, "one agent, its action computed by the env's first lanes");
    __shared__ Shared<L> sh;
    extern __shared__ float4 policy_lds4[];
    float* const lds = reinterpret_cast<float*>(policy_lds4);
#ifdef RSX_TIMING
    if (threadIdx.x == 0) sh.dbg = nullptr;
#endif
    const int n_steps = n_steps_arg & RSX_N_STEPS_MASK;
    // the step counter of this launch (rsx_hot_args.hpp: step_tick): every workgroup of the grid takes part, the idle tail included
    const bool tick_dev = (n_steps_arg & RSX_TICK_DEV) != 0;
    const StepTick tk = step_tick(tick_dev, P, bufs, (uint32_t)n_steps);
    if (__builtin_expect(!tk.ok, 0)) return;
    const uint32_t tick0 = tk.t;
    const int lane = threadIdx.x;
    const int b = LaneMap<L>::body(lane), g = LaneMap<L>::env(lane);
    const int tile = tile_of_block(per_xcd);
    if (tile * G >= P.num_envs) return;   // the idle tail behind the last tile: its slot is advanced, nothing else is its to do
    const int e = tile * G + g;
    const int N = NR ? NR : P.n_robots;
    const bool live = e < P.num_envs;
    const bool is_robot = live && b < N, is_ball = live && b == N;
    const size_t B = (size_t)P.num_envs;
    const uint32_t env_id = P.env_id_base + (uint32_t)e;
    constexpr int OD_C = obs_dim_c<TASK, NR>();
    const int OD = OD_C ? OD_C : P.obs_dim;
#define auxe(ROW) at_byte(bufs.aux, (ix_t)(ROW) * ((ix_t)4 * (ix_t)P.row_stride) + (ix_t)4 * (ix_t)e)   // row ROW of this env in the scalar arena

    // ---- the policy's weights -> LDS, once (the output layer 2 AD units wide); the env's current observation -> its row ----
    const PolicyImage m = gaussian_image(G, OD, AD, Q.layers, Q.hidden);
    stage_policy(params, lds, m, Q, OD, 2 * AD, lane);
    float* const row = lds + m.rows + g * m.xs;              // this env's observation
    float* const oa = lds + m.rows + 3 * G * m.xs + g * 8;   // ... and the action the policy answers with
    for (int i = b; i < OD; i += L) row[i] = live ? bufs.obs[(size_t)e * OD + i] : 0.0f;
    const bool noisy = C.deterministic == 0;   // (uniform: a launch argument)

    // ---- load: the env's state and task scalars, once (as rsx_task_step_body.inc) ----
    Body o; float od, wd, wheels[4];
    const RawBody raw = load_raw<KIND>(P, bufs.state, e, b, is_robot, is_ball);
    std::conditional_t<PHYS, EnvCoef, LitCoef<KIND>> cf{};
    if constexpr (PHYS) if (live) load_coefs(P, phys, e, cf);
    int steps = 0; uint32_t episode = 0;
    if (live) {
        steps = __float_as_int(auxe(ROW_STEPS));
        episode = __float_as_uint(auxe(ROW_EPISODE));
    }
    float ou0 = 0.0f, ou1 = 0.0f;
    if (TASK == RSX_TASK_VSS_V0 && is_robot && b >= 1) {
        ou0 = auxe(ROW_OU + 2 * b); ou1 = auxe(ROW_OU + 2 * b + 1);
    }
    float info[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    float prev_pot = 0.0f, ep_ret = 0.0f;
#include "rsx_step_ball_load.inc"
    // metrics[0] (env-steps): counted by ONE lane of the grid, a plain read-modify-write (launches of a handle are stream-ordered)
    const bool counts_steps = blockIdx.x == 0 && lane == 0;
    unsigned long long steps_before = 0;
    if (counts_steps) steps_before = bufs.metrics[0];
    float reward = 0.0f; int term = 0, trunc = 0;
    bool success = false;  // goal scored / course completed / pass received (metrics[2])
    bool against = false;  // goal conceded (metrics[3])
    bool was_reset = false;
    const bool commands = is_robot && b == 0;
    constexpr bool fed = true;   // every step's action is the policy's: the shared fragments and draw_for_step never draw the agent's
    float act[AD];
#pragma unroll
    for (int i = 0; i < AD; ++i) act[i] = 0.0f;

    // All loads land here, once (see the head of rsx_collect.hip)
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    interpret_body<KIND>(raw, is_robot, is_ball, o, od, wd, wheels);
    // VSS-v0's task scalar is a function of the ball's position (rsx_collect.hip explains why it is derived here)
    if (TASK == RSX_TASK_VSS_V0 && is_ball) prev_pot = vss_ball_potential(o.x, o.y, P.hl_goal, P.inv_len_cm);
    wave_sync();   // weights and rows are in place

    for (int it = 0; it < n_steps; ++it) {
        const uint32_t t = tick0 + (uint32_t)it;   // per-step draws are keyed by the handle's step count, not by the env's counters
        const size_t rec = (size_t)it * B + (size_t)e;   // this step's row of this env in every output
        // ---- a_t = tanh(mu + exp(clamp(raw)) * eps) of obs_t: the row the previous step (or the handle) left ----
        if (live)
            for (int i = b; i < OD; i += L) obs_out[rec * (size_t)OD + i] = row[i];
        float raw_ls;
        const float mean = Q.hidden == 64 ? gaussian_forward<64, L, AD>(lds, m, Q, OD, b, g, raw_ls)
                                          : gaussian_forward<32, L, AD>(lds, m, Q, OD, b, g, raw_ls);
        if (b < AD) {
            const float ls = clampf(raw_ls, C.ls_min, C.ls_max);
            float smp = mean;
            if (noisy) {
                // component b takes normal b & 3 of block b >> 2: rsx_collect.hip's draw, unchanged
                const u32x4 u = philox4x32(env_id, 0u, t, DOM_POLICY | ((uint32_t)(b >> 2) << 8), C.k0, C.k1);
                float n0, n1;
                plan_normal_pair((b & 2) ? u.z : u.x, (b & 2) ? u.w : u.y, n0, n1);
                const float eps = (b & 1) ? n1 : n0;
                const float sigma = exp_f32(ls);
                smp = mean + sigma * eps;   // (two roundings: the unit is built with -ffp-contract=off)
            }
            const float a = tanh_f32(smp);
            oa[b] = a;
            if (live) {
                act_out[rec * (size_t)AD + b] = a;
                if (C.mean != nullptr) C.mean[rec * (size_t)AD + b] = mean;
                if (C.sample != nullptr) C.sample[rec * (size_t)AD + b] = smp;
                if (C.log_std != nullptr) C.log_std[rec * (size_t)AD + b] = ls;
            }
        }
        wave_sync();
        if (commands) {
#pragma unroll
            for (int i = 0; i < AD; ++i) act[i] = oa[i];
        }

        // ---- the step: rsx_task_step_body.inc's stepping trip ----
        bool ended;
        const float obs_ts = prev_pot;   // the task scalar as this step's observation sees it (before the reward moves it)
        const bool first_step = steps == 0;
        if (is_ball && first_step) {
#pragma unroll
            for (int i = 0; i < 10; ++i) info[i] = 0.0f;
            ep_ret = 0.0f;
        }
        const float lastx = o.x, lasty = o.y;  // the reference's last_frame (pre-step)

        // ---- actions -> commands ----
        float q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const StepDraw dr = draw_for_step<KIND, TASK>(P, env_id, t, b, is_robot, fed);
#include "rsx_step_commands.inc"

        // ---- physics ----
        physics<KIND, L, NR>(P, o, b, g, live, sh, cf);

        // ---- wire-format values, the observation the next step's action answers, reward ----
#include "rsx_step_wire.inc"
        write_obs<KIND, TASK>(P, row, b, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd, o.ir, obs_ts);
#include "rsx_step_xr.inc"
        wave_sync();
#include "rsx_step_reward.inc"
        if (is_ball) {
            C.rewards[rec] = reward;
            C.flags[rec] = (uint8_t)(term | (trunc << 1));
        }

        // ---- episode end: same-step auto-reset ----
        if (RSX_RARE_B(KIND, 4, __any(ended))) {
            if (ended) {  // terminal observation
                write_obs<KIND, TASK>(P, bufs.final_obs + (size_t)e * OD, b, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd, o.ir, obs_ts);
                if (C.final_obs != nullptr)
                    write_obs<KIND, TASK>(P, C.final_obs + rec * (size_t)OD, b, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd, o.ir, obs_ts);
                episode += 1;   // every lane of the env: the new episode's id
            }
            if (KIND == RSX_KIND_VSS) {
#include "rsx_step_vss_metrics.inc"
            } else {
                // SSL tasks: the ball lane holds the increments, lanes 0..5 of the env add one each (see the body)
                static_assert(KIND == RSX_KIND_VSS || L >= 6, "metrics fan-out needs 6 lanes per env");
                uint32_t* const mv = reinterpret_cast<uint32_t*>(sh.x0[g]);   // 12 words, free again after the reward
                if (ended && is_ball) {
                    unsigned long long inc[6];
                    inc[0] = 1ull;
                    inc[1] = success ? 1ull : 0ull;
                    inc[2] = against ? 1ull : 0ull;
                    inc[3] = (unsigned long long)__float2ll_rn(ep_ret * 1048576.0f);
                    inc[4] = (unsigned long long)steps;
                    inc[5] = (trunc && !term) ? 1ull : 0ull;
#pragma unroll
                    for (int k = 0; k < 6; ++k) { mv[2 * k] = (uint32_t)inc[k]; mv[2 * k + 1] = (uint32_t)(inc[k] >> 32); }
                }
                wave_sync();
                if (ended && b < 6) {
                    const unsigned long long v = (unsigned long long)mv[2 * b] | ((unsigned long long)mv[2 * b + 1] << 32);
                    if (v) atomicAdd(&metric_slot(bufs)[1 + b], v);
                }
            }
            // placement: the sequential form of the multi-step launches (a launch of many steps pays for the average wave)
            if (ended) place_predraw<TASK, L>(P, env_id, episode, b, sh.draws[g]);
            wave_sync();  // draws published; stage rows of ended envs are about to be overwritten
            float4 pz = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (ended && is_ball) place_env<TASK, L>(P, N, env_id, episode, g, sh.A, sh.draws[g]);
            wave_sync();
            if (ended && (is_robot || is_ball)) pz = sh.A[LaneMap<L>::slot(b, g)];
            if (ended) {
                steps = 0; ou0 = 0.0f; ou1 = 0.0f; was_reset = true;
                if constexpr (PHYS) phys_redraw(P, phys, e, env_id, episode, b == 0, cf);
                if (TASK >= RSX_TASK_SSL_DRIBBLING) prev_pot = 0.0f;  // checkpoints_count / stopped_steps
                if (is_robot || is_ball) {
                    o = Body{};
                    o.x = pz.x; o.y = pz.y;
                    od = pz.z; wd = 0.0f;
                    wheels[0] = wheels[1] = wheels[2] = wheels[3] = 0.0f;
                    if (is_robot) { o.th = od; sincos_f32(o.th * K::deg2rad, o.s, o.c); }
                }
                // the first observation of the next episode: what the next step's action answers, row t + 1 of the record
                write_obs<KIND, TASK>(P, row, b, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd, 0, 0.0f);
            }
            wave_sync();
        }

        wave_sync();
    }

    // ---- store: the state in wire format, the scalars, and the last observation into the handle's obs buffer ----
    store_body<KIND>(P, bufs.state, e, b, is_robot, is_ball, o, od, wd, wheels, P.n_sub != 0 || was_reset);
    if (live) {
        for (int i = b; i < OD; i += L) bufs.obs[(size_t)e * OD + i] = row[i];
        if (b == 0) {
            auxe(ROW_STEPS) = __int_as_float(steps);
            auxe(ROW_EPISODE) = __uint_as_float(episode);
        }
    }
    if (TASK == RSX_TASK_VSS_V0 && is_robot && b >= 1) {
        auxe(ROW_OU + 2 * b) = ou0; auxe(ROW_OU + 2 * b + 1) = ou1;
    }
    if (is_ball) {
        auxe(ROW_PREV_POT) = prev_pot;
        if (TASK != RSX_TASK_VSS_V0) auxe(ROW_EP_RET) = ep_ret;
    }
#undef auxe
    if (counts_steps) bufs.metrics[0] = steps_before + (unsigned long long)P.num_envs * (unsigned long long)n_steps;
}

template <bool PHYS>
void gaussian_launch(const Params& P, const Buffers& b, const int L, const int NR, float* phys, const PolicyArgs& Q, const GaussianArgs& C,
                     const int act_dim, const int n_steps, hipStream_t s) {
    const int grid = lane_grid(L, P.num_envs);
    with_task(P.task, [&](auto kind, auto task, auto nrs, auto fixed) {
        if constexpr (task != RSX_TASK_SSL_SCRIMMAGE) {   // (the scrimmage commands every robot: refused by the caller)
            with_task_variant<task, nrs, fixed, 32>(L, NR, [&](auto l, auto nr) {   // (64 lanes per env: refused by the caller)
                const size_t lds = sizeof(float) * (size_t)gaussian_image(64 / l, P.obs_dim, act_dim, Q.layers, Q.hidden).total;
                rsx_launch((task_collect_gaussian_kernel<kind, task, l, nr, PHYS>), dim3((unsigned)grid), dim3(64), lds, s, Q.params, C.obs,
                           C.actions, grid >> 3, n_steps, P, b, Q, C, phys);
            });
        }
    });
}

template <int L> constexpr size_t static_lds() { return sizeof(Shared<L>); }

}  // namespace

long long gaussian_lds_bytes(const int L, const int obs_dim, const int act_dim, const PolicySpec& p) {
    const size_t fixed = L == 8 ? static_lds<8>() : L == 16 ? static_lds<16>() : static_lds<32>();
    return (long long)fixed + 4ll * (long long)gaussian_image(64 / L, obs_dim, act_dim, p.layers, p.hidden).total;
}

void launch_task_collect_gaussian(const Params& P, const Buffers& b, const int L, const int NR, float* phys, const PolicySpec& p,
                                  const float* params, const int n_params, const int act_dim, const rsx_collect_gaussian_cfg& cfg,
                                  const int n_steps, const rsx_collect_out& out, float* log_std_out, hipStream_t s) {
    const PolicyArgs Q{params, b.obs, nullptr, nullptr, n_params, p.layers, p.hidden, p.hidden_act, p.out_act};
    const GaussianArgs C{out.obs, out.actions, out.rewards, out.flags, out.final_obs, out.mean, out.sample, log_std_out,
                         cfg.log_std_min, cfg.log_std_max, cfg.deterministic, (uint32_t)cfg.noise_seed, (uint32_t)(cfg.noise_seed >> 32)};
    if (phys) gaussian_launch<true>(P, b, L, NR, phys, Q, C, act_dim, n_steps, s);
    else gaussian_launch<false>(P, b, L, NR, nullptr, Q, C, act_dim, n_steps, s);
}

}  // namespace rsx
