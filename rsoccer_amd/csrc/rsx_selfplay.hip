// rsx_selfplay.hip — self-play collection for VSS-v0: rsx_collect.hip's launch with yellow robot 0 (body index n_blue) driven by a second
// MLP policy, the opponent, evaluated inside the same launch from the mirrored observation (include/rsx.h: rsx_task_collect_selfplay).
// A translation unit of its own, a sibling of rsx_collect.hip, so that the instantiations of every existing kernel — the collector's
// included — stay exactly what they were.
//
// task_collect_selfplay_kernel follows the loop of task_collect_policy_kernel piece by piece (the same step pieces and text fragments,
// the same stores, the same auto-reset) and adds:
//   a second PolicyImage      staged in LDS behind the first (rsx_policy_mlp.hpp: policy_image, stage_policy), with rows and an action
//                             slot of its own; the two policies may differ in layers and hidden;
//   the mirrored observation  its row per env is the first row of the second image, filled by write_obs_mirrored next to every
//                             write_obs of the agent's row, from the same registers: row t of both describes the same instant;
//   the opponent's forward    policy_forward on the second image, by the lanes of the env, before the agent's action is applied: both
//                             policies answer observation t;
//   its head                  the agent's recipe under a Philox domain word of its own (DOM_OPPONENT): the heads never share a draw;
//   the command               behind rsx_step_commands.inc the lane of body n_blue overwrites q[0], q[1] with vss_wheel of the two
//                             outputs and redoes robot_targets.  Its Ornstein-Uhlenbeck state has advanced on its usual draws in the
//                             fragment, unused: the env can be handed back to rsx_task_step / rsx_task_collect_policy at any time.
// Reward, flags, metrics, final_obs and the handle's obs buffer stay the agent's (blue's).
//
// Grid: the handle's lane-group grid (lane_grid), one 64-lane workgroup per tile.
// LDS per workgroup: Shared<L> + two images.  VSS-v0 3v3 at 8 lanes per env, 40-64-64-2 on both sides: 2 x 36 384 B + 6 272 B static =
// 79 040 B, i.e. TWO workgroups (two waves) per CU of the 163 840 B, against three for the collector — 512 resident workgroups on 256
// CUs, which is what 4096 envs need; 5v5 at 16 lanes per env (64-64-64-2 twice): 2 x 39 520 B + 5 568 B = 84 608 B, ONE workgroup per CU.
// Registers do not limit either (one wave per workgroup).  More than 64 KB of dynamic LDS: the launch raises the kernel's limit first
// (selfplay_launch); the host refuses images that pass the 160 KB of a CU.
//
// Memory traffic of the loop: stores only, as in rsx_collect.hip.  Every load — both policies' weights, state, scalars, the observation
// row, both sigmas — is issued ahead of the loop and lands behind ONE vmcnt(0).
#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

#include "rsx.h"
#include "rsx_plan_common.hpp"
#include "rsx_policy_mlp.hpp"
#include "rsx_seats.hpp"
#include "rsx_units.hpp"
#include "rsx_variants.hpp"

namespace rsx {

namespace {

// OPPONENT: the noise of the opponent's Gaussian head, counter (env, 0, tick, OPPONENT | block << 8), keyed by the call's noise_seed like
// the agent's (rsx_math.hpp: DOM_POLICY = 7; rsx_ppo_update.hip: DOM_PERM = 8)
constexpr uint32_t DOM_OPPONENT = 9u;

struct CollectArgs {   // (as rsx_collect.hip's)
    float* obs;            // [T][B][obs_dim]
    float* actions;        // [T][B][act_dim]
    float* rewards;        // [T][B]
    uint8_t* flags;        // [T][B] bit 0 terminated, bit 1 truncated
    float* final_obs;      // [T][B][obs_dim] or nullptr: rows of ended (t, env) only
    float* mean;           // [T][B][act_dim] or nullptr
    float* sample;         // [T][B][act_dim] or nullptr
    const float* sigma;    // [act_dim] or nullptr = deterministic
    uint32_t k0, k1;       // noise_seed lo, hi: the Philox key of both heads' noise
};

struct SelfplayArgs {
    const float* params;   // the opponent's parameters [P2]
    const float* sigma;    // [2] or nullptr = deterministic
    float* obs;            // [T][B][obs_dim] or nullptr: the mirrored observation each opponent action answered
    float* actions;        // [T][B][2] or nullptr
    float* mean;           // [T][B][2] or nullptr
    float* sample;         // [T][B][2] or nullptr
};

// (the mirrored row, write_obs_mirrored: rsx_seats.hpp)

// one component of a Gaussian head (rsx_collect.hip's, with the domain word a parameter): component b takes normal b & 3 of block b >> 2
__device__ __forceinline__ float head_sample(const float mean, const float sigma, const uint32_t env_id, const uint32_t t, const int b,
                                             const uint32_t dom, const uint32_t k0, const uint32_t k1) {
    const u32x4 u = philox4x32(env_id, 0u, t, dom | ((uint32_t)(b >> 2) << 8), k0, k1);
    float n0, n1;
    plan_normal_pair((b & 2) ? u.z : u.x, (b & 2) ? u.w : u.y, n0, n1);
    const float eps = (b & 1) ? n1 : n0;
    return mean + sigma * eps;   // (two roundings: the unit is built with -ffp-contract=off)
}

template <int KIND, int TASK, int L, int NR, bool PHYS>
__global__ __launch_bounds__(64) void task_collect_selfplay_kernel(const float* __restrict__ params, const float* __restrict__ sigma_dev,
                                                                   float* __restrict__ obs_out, float* __restrict__ act_out,
                                                                   const int per_xcd, const int n_steps_arg, const Params P,
                                                                   const Buffers bufs, const PolicyArgs Q, const PolicyArgs Q2,
                                                                   const CollectArgs C, const SelfplayArgs S, float* phys) {
    using K = KC<KIND>;
    using T = TC<TASK>;
    constexpr int G = 64 / L;
    constexpr int ID = T::info_dim;
    constexpr int AD = T::act_dim;
    constexpr int MODE = MODE_ROLLOUT;   // (what the shared fragments specialise on: the multi-step trip)
    constexpr int mode = 0;
    static_assert(KIND == RSX_KIND_VSS && TASK == RSX_TASK_VSS_V0 && AD == 2 && AD <= L, "VSS-v0 only: yellow 0 takes two wheel commands");
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
    const int NB = NR ? NR / 2 : P.n_blue;   // equal teams (checked by the host)
    const bool live = e < P.num_envs;
    const bool is_robot = live && b < N, is_ball = live && b == N;
    const size_t B = (size_t)P.num_envs;
    const uint32_t env_id = P.env_id_base + (uint32_t)e;
    constexpr int OD_C = obs_dim_c<TASK, NR>();
    const int OD = OD_C ? OD_C : P.obs_dim;
#define auxe(ROW) at_byte(bufs.aux, (ix_t)(ROW) * ((ix_t)4 * (ix_t)P.row_stride) + (ix_t)4 * (ix_t)e)   // row ROW of this env in the scalar arena

    // ---- both policies' weights -> LDS, once; the env's current observation -> its row; the heads' sigmas ----
    const PolicyImage m = policy_image(G, OD, AD, Q.layers, Q.hidden);
    const PolicyImage m2 = policy_image(G, OD, AD, Q2.layers, Q2.hidden);
    float* const lds2 = lds + m.total;   // (a multiple of 4 floats: the second image is 16-byte aligned like the first)
    stage_policy(params, lds, m, Q, OD, AD, lane);
    stage_policy(S.params, lds2, m2, Q2, OD, AD, lane);
    float* const row = lds + m.rows + g * m.xs;                // this env's observation
    float* const oa = lds + m.rows + 3 * G * m.xs + g * 8;     // ... and the action the agent answers with
    float* const row2 = lds2 + m2.rows + g * m2.xs;            // the mirrored observation
    float* const oa2 = lds2 + m2.rows + 3 * G * m2.xs + g * 8; // ... and the opponent's answer
    for (int i = b; i < OD; i += L) row[i] = live ? bufs.obs[(size_t)e * OD + i] : 0.0f;
    if (!live)
        for (int i = b; i < OD; i += L) row2[i] = 0.0f;
    const bool noisy = sigma_dev != nullptr, noisy2 = S.sigma != nullptr;   // (uniform: launch arguments)
    float sigma = 0.0f, sigma2 = 0.0f;
    if (noisy && b < AD) sigma = sigma_dev[b];
    if (noisy2 && b < AD) sigma2 = S.sigma[b];

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
    if (is_robot && b >= 1) {
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
    bool success = false;  // goal scored (metrics[2])
    bool against = false;  // goal conceded (metrics[3])
    bool was_reset = false;
    const bool commands = is_robot && b == 0;
    const bool opposes = is_robot && b == NB;   // yellow 0
    constexpr bool fed = true;   // every step's action is the policy's: the shared fragments and draw_for_step never draw the agent's
    float act[AD];
#pragma unroll
    for (int i = 0; i < AD; ++i) act[i] = 0.0f;

    // All loads land here, once (see the head of this file)
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    interpret_body<KIND>(raw, is_robot, is_ball, o, od, wd, wheels);
    // the task scalar is a function of the ball's position (rsx_collect.hip explains why it is derived here)
    if (is_ball) prev_pot = vss_ball_potential(o.x, o.y, P.hl_goal, P.inv_len_cm);
    // the mirrored row of step 0: from the state the handle's obs row was written from (the wire format is what both start from)
    write_obs_mirrored(P, row2, b, NB, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd);
    wave_sync();   // weights and rows are in place

    for (int it = 0; it < n_steps; ++it) {
        const uint32_t t = tick0 + (uint32_t)it;   // per-step draws are keyed by the handle's step count, not by the env's counters
        const size_t rec = (size_t)it * B + (size_t)e;   // this step's row of this env in every output
        // ---- a_t = head(policy(obs_t)) and the opponent's head(opponent(mirrored obs_t)): both answer the rows the previous step left ----
        if (live) {
            for (int i = b; i < OD; i += L) obs_out[rec * (size_t)OD + i] = row[i];
            if (S.obs != nullptr)
                for (int i = b; i < OD; i += L) S.obs[rec * (size_t)OD + i] = row2[i];
        }
        const float mean = Q.hidden == 64 ? policy_forward<64, L, AD, false>(lds, m, Q, OD, b, g)
                                          : policy_forward<32, L, AD, false>(lds, m, Q, OD, b, g);
        const float mean2 = Q2.hidden == 64 ? policy_forward<64, L, AD, false>(lds2, m2, Q2, OD, b, g)
                                            : policy_forward<32, L, AD, false>(lds2, m2, Q2, OD, b, g);
        if (b < AD) {
            const float smp = noisy ? head_sample(mean, sigma, env_id, t, b, DOM_POLICY, C.k0, C.k1) : mean;
            const float smp2 = noisy2 ? head_sample(mean2, sigma2, env_id, t, b, DOM_OPPONENT, C.k0, C.k1) : mean2;
            const float a = policy_act(smp, Q.out_act), a2 = policy_act(smp2, Q2.out_act);
            oa[b] = a;
            oa2[b] = a2;
            if (live) {
                act_out[rec * (size_t)AD + b] = a;
                if (C.mean != nullptr) C.mean[rec * (size_t)AD + b] = mean;
                if (C.sample != nullptr) C.sample[rec * (size_t)AD + b] = smp;
                if (S.actions != nullptr) S.actions[rec * (size_t)AD + b] = a2;
                if (S.mean != nullptr) S.mean[rec * (size_t)AD + b] = mean2;
                if (S.sample != nullptr) S.sample[rec * (size_t)AD + b] = smp2;
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

        // ---- actions -> commands; yellow 0's is the opponent's (its OU state has advanced in the fragment, unused) ----
        float q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const StepDraw dr = draw_for_step<KIND, TASK>(P, env_id, t, b, is_robot, fed);
#include "rsx_step_commands.inc"
        if (opposes) {
            q[0] = vss_wheel(oa2[0]); q[1] = vss_wheel(oa2[1]);
            robot_targets<KIND>(P, o, q);
        }

        // ---- physics ----
        physics<KIND, L, NR>(P, o, b, g, live, sh, cf);

        // ---- wire-format values, the observations the next step's actions answer, reward ----
#include "rsx_step_wire.inc"
        write_obs<KIND, TASK>(P, row, b, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd, o.ir, obs_ts);
        write_obs_mirrored(P, row2, b, NB, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd);
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
#include "rsx_step_vss_metrics.inc"
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
                if (is_robot || is_ball) {
                    o = Body{};
                    o.x = pz.x; o.y = pz.y;
                    od = pz.z; wd = 0.0f;
                    wheels[0] = wheels[1] = wheels[2] = wheels[3] = 0.0f;
                    if (is_robot) { o.th = od; sincos_f32(o.th * K::deg2rad, o.s, o.c); }
                }
                // the first observations of the next episode: what the next step's actions answer, row t + 1 of the records
                write_obs<KIND, TASK>(P, row, b, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd, 0, 0.0f);
                write_obs_mirrored(P, row2, b, NB, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd);
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
    if (is_robot && b >= 1) {
        auxe(ROW_OU + 2 * b) = ou0; auxe(ROW_OU + 2 * b + 1) = ou1;
    }
    if (is_ball) auxe(ROW_PREV_POT) = prev_pot;
#undef auxe
    if (counts_steps) bufs.metrics[0] = steps_before + (unsigned long long)P.num_envs * (unsigned long long)n_steps;
}

template <int L> constexpr size_t static_lds() { return sizeof(Shared<L>); }

// dynamic LDS of one workgroup: the two images back to back
size_t images_bytes(const int L, const int obs_dim, const int act_dim, const PolicySpec& a, const PolicySpec& o) {
    return sizeof(float) * ((size_t)policy_image(64 / L, obs_dim, act_dim, a.layers, a.hidden).total +
                            (size_t)policy_image(64 / L, obs_dim, act_dim, o.layers, o.hidden).total);
}

template <bool PHYS>
void selfplay_launch(const Params& P, const Buffers& b, const int L, const int NR, float* phys, const PolicyArgs& Q, const PolicyArgs& Q2,
                     const CollectArgs& C, const SelfplayArgs& S, const int act_dim, const int n_steps, hipStream_t s) {
    const int grid = lane_grid(L, P.num_envs);
    const size_t lds = images_bytes(L, P.obs_dim, act_dim, PolicySpec{Q.layers, Q.hidden, Q.hidden_act, Q.out_act},
                                    PolicySpec{Q2.layers, Q2.hidden, Q2.hidden_act, Q2.out_act});
    with_task_variant<RSX_TASK_VSS_V0, 6, false, 32>(L, NR, [&](auto l, auto nr) {   // (64 lanes per env: refused by the caller)
        const auto kernel = task_collect_selfplay_kernel<RSX_KIND_VSS, RSX_TASK_VSS_V0, l, nr, PHYS>;
        // dynamic LDS beyond 64 KB is the kernel's to be granted first: once per variant and device, and again for a larger image
        static std::atomic<int> granted[64];
        int dev = 0;
        if (lds > 65536 && hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 && granted[dev].load(std::memory_order_relaxed) < (int)lds) {
            const hipError_t rc = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (rc == hipSuccess) granted[dev].store((int)lds, std::memory_order_relaxed);
            else if (g_launch_status == hipSuccess) g_launch_status = rc;
        }
        rsx_launch(kernel, dim3((unsigned)grid), dim3(64), lds, s, Q.params, C.sigma, C.obs, C.actions, grid >> 3, n_steps, P, b, Q, Q2, C, S,
                   phys);
    });
}

}  // namespace

long long selfplay_lds_bytes(const int L, const int obs_dim, const int act_dim, const PolicySpec& agent, const PolicySpec& opponent) {
    const size_t fixed = L == 8 ? static_lds<8>() : L == 16 ? static_lds<16>() : static_lds<32>();
    return (long long)fixed + (long long)images_bytes(L, obs_dim, act_dim, agent, opponent);
}

void launch_task_collect_selfplay(const Params& P, const Buffers& b, const int L, const int NR, float* phys, const PolicySpec& p,
                                  const float* params, const int n_params, const PolicySpec& opp, const float* opp_params,
                                  const int n_opp_params, const int act_dim, const float* sigma, const float* opp_sigma,
                                  const uint64_t noise_seed, const int n_steps, const rsx_collect_out& out, const rsx_selfplay_out& sp,
                                  hipStream_t s) {
    const PolicyArgs Q{params, b.obs, nullptr, nullptr, n_params, p.layers, p.hidden, p.hidden_act, p.out_act};
    const PolicyArgs Q2{opp_params, b.obs, nullptr, nullptr, n_opp_params, opp.layers, opp.hidden, opp.hidden_act, opp.out_act};
    const CollectArgs C{out.obs, out.actions, out.rewards, out.flags, out.final_obs, out.mean, out.sample, sigma, (uint32_t)noise_seed,
                        (uint32_t)(noise_seed >> 32)};
    const SelfplayArgs S{opp_params, opp_sigma, sp.opp_obs, sp.opp_actions, sp.opp_mean, sp.opp_sample};
    if (phys) selfplay_launch<true>(P, b, L, NR, phys, Q, Q2, C, S, act_dim, n_steps, s);
    else selfplay_launch<false>(P, b, L, NR, nullptr, Q, Q2, C, S, act_dim, n_steps, s);
}

}  // namespace rsx
