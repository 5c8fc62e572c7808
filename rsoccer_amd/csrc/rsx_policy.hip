// rsx_policy.hip — closed-loop lookahead: MLP policies evaluated inside the exact lookahead launch (include/rsx.h:
// rsx_task_lookahead_policy), in a translation unit of its own so that the instantiations of every existing kernel stay exactly
// what they were.
//
// task_lookahead_policy_kernel is task_lookahead_kernel (rsx_plan.hip) with another action source: per (env, policy) pair it runs up
// to `horizon` fused task steps from the env's CURRENT state, and the action of step t is the policy's answer to the observation
// the pair itself produced at step t - 1 (step 0: the env's row of the handle's obs buffer).  The step is built from the pieces the
// lookahead is built from — load_raw, interpret_body, draw_for_step, physics, write_obs, task_reward and the three text fragments
// rsx_step_commands.inc, rsx_step_wire.inc, rsx_step_xr.inc — so with the same actions both compute the same floats: feeding this
// kernel's recorded actions to rsx_task_lookahead gives its returns, steps, flags and last observation bit for bit.  The loop is
// this unit's own and not rsx_plan_body.inc: that body fetches the action of step it + 1 while step it computes, which a policy
// cannot do, and a hook for it would have to be shown not to move an instruction of the two kernels that include it.
//
// Grid: rsx_plan.hip's — one 64-lane workgroup per (tile, policy), runs of K consecutive workgroups per tile, a pure function of the
// grid.  The workgroup's policy is the same for all its envs; how its weights lie in LDS and how a lane evaluates its units is
// rsx_policy_mlp.hpp's, shared with the on-policy collector (rsx_collect.hip).
//
// LDS per workgroup: Shared<L> + weights + three rows per env (policy_lds_bytes below; VSS-v0 3v3 with 2 x 64 units: 41 KB, so three
// single-wave workgroups share a CU's 160 KB).  The host refuses a policy whose image passes 64 KB (generic variants on large fields).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rsx.h"
#include "rsx_plan_common.hpp"
#include "rsx_policy_mlp.hpp"
#include "rsx_units.hpp"
#include "rsx_variants.hpp"

namespace rsx {

namespace {

template <int KIND, int TASK, int L, int NR, bool PHYS>
__global__ __launch_bounds__(64) void task_lookahead_policy_kernel(float* __restrict__ returns, int32_t* __restrict__ steps_out,
                                                                   uint8_t* __restrict__ flags_out, float* __restrict__ last_obs,
                                                                   const int per_xcd, const Params P, const PlanArgs A, const PolicyArgs Q,
                                                                   const float* __restrict__ phys) {
    using K = KC<KIND>;
    using T = TC<TASK>;
    constexpr int G = 64 / L;
    constexpr int ID = T::info_dim;
    constexpr int AD = T::act_dim;
    static_assert(TASK != RSX_TASK_SSL_SCRIMMAGE && AD <= 8 && AD <= L, "one agent, its action computed by the env's first lanes");
    __shared__ Shared<L> sh;
    extern __shared__ float4 policy_lds4[];
    float* const lds = reinterpret_cast<float*>(policy_lds4);
#ifdef RSX_TIMING
    if (threadIdx.x == 0) sh.dbg = nullptr;
#endif
    const int lane = threadIdx.x;
    const int b = LaneMap<L>::body(lane), g = LaneMap<L>::env(lane);
    // (tile, policy) of this workgroup: rsx_plan.hip's mapping
    const int v = tile_of_block(per_xcd);
    const int tile = v / A.n_cand, k = v - tile * A.n_cand;
    const int e = tile * G + g;
    const int N = NR ? NR : P.n_robots;
    const bool live = e < P.num_envs;
    const uint32_t env_id = P.env_id_base + (uint32_t)e;
    constexpr int OD_C = obs_dim_c<TASK, NR>();
    const int OD = OD_C ? OD_C : P.obs_dim;
#define auxe(ROW) at_byte(A.aux, (ix_t)(ROW) * ((ix_t)4 * (ix_t)P.row_stride) + (ix_t)4 * (ix_t)e)   // row ROW of this env in the scalar arena
    const size_t pair = (size_t)e * (size_t)A.n_cand + (size_t)k;   // row of this pair in every output

    // ---- the policy's weights -> LDS, once; the env's current observation -> its row ----
    const PolicyImage m = policy_image(G, OD, AD, Q.layers, Q.hidden);
    {
        const float* w = Q.params + (size_t)k * (size_t)Q.n_params;
        const int H = Q.hidden;
        stage_layer(w, H, OD, lds + m.w1, m.ws, lds + m.b1, lane);
        w += (size_t)H * OD + H;
        if (Q.layers == 2) {
            stage_layer(w, H, H, lds + m.w2, m.ws, lds + m.b2, lane);
            w += (size_t)H * H + H;
        }
        stage_layer(w, AD, H, lds + m.wo, m.as, lds + m.bo, lane);
    }
    float* const row = lds + m.rows + g * m.xs;         // this env's observation
    float* const oa = lds + m.rows + 3 * G * m.xs + g * 8;   // ... and the action the policy answers with
    for (int i = b; i < OD; i += L) row[i] = live ? Q.obs[(size_t)e * OD + i] : 0.0f;

    // ---- load: the env's state and task scalars, once (as rsx_plan_body.inc) ----
    bool is_robot = live && b < N, is_ball = live && b == N;
    Body o; float od, wd, wheels[4];
    const RawBody raw = load_raw<KIND>(P, A.state, e, b, is_robot, is_ball);
    std::conditional_t<PHYS, EnvCoef, LitCoef<KIND>> cf{};
    if constexpr (PHYS) if (live) load_coefs(P, phys, e, cf);
    int steps = 0;
    if (live) steps = __float_as_int(auxe(ROW_STEPS));
    float ou0 = 0.0f, ou1 = 0.0f;
    if (TASK == RSX_TASK_VSS_V0 && is_robot && b >= 1) {
        ou0 = auxe(ROW_OU + 2 * b); ou1 = auxe(ROW_OU + 2 * b + 1);
    }
    float info[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    float prev_pot = 0.0f;
    if (is_ball) {
#pragma unroll
        for (int i = 0; i < ID; ++i)
            if (!(TASK == RSX_TASK_VSS_V0 && (i == 0 || i >= 4))) info[i] = auxe(ROW_INFO + i);
        if (TASK != RSX_TASK_VSS_V0) prev_pot = auxe(ROW_PREV_POT);   // (VSS-v0: derived from the ball's position below)
    }
#undef auxe
    // the handle's step counter, not advanced; a counter that `horizon` more steps would wrap: nothing is simulated
    uint32_t tick0 = P.tick_base;
    int horizon = A.horizon;
    if (A.ticks != nullptr) {
        tick0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.ticks[0]);
        if (tick0 > 0xFFFFFFFFu - (uint32_t)horizon) horizon = 0;
    }
    const bool commands = is_robot && b == 0;
    constexpr bool fed = true;   // every step's action is the policy's: the shared fragments and draw_for_step never draw the agent's
    float act[AD];
#pragma unroll
    for (int i = 0; i < AD; ++i) act[i] = 0.0f;
    interpret_body<KIND>(raw, is_robot, is_ball, o, od, wd, wheels);
    if (TASK == RSX_TASK_VSS_V0 && is_ball) prev_pot = vss_ball_potential(o.x, o.y, P.hl_goal, P.inv_len_cm);   // (see rsx_plan_body.inc)

    // per-pair results, held by every lane of the pair (the ball lane's copy is the one that counts)
    float ret = 0.0f, disc = 1.0f;
    int n_sim = 0, fl = 0;
    bool alive = live;   // the pair's env has not ended yet
    wave_sync();         // weights and rows are in place

    for (int it = 0; it < horizon; ++it) {
        if (!__any(alive)) break;   // every env of the wave has ended (or the tile holds none)
        // ---- a_t = policy(obs_t): obs_t is the row the previous step (or the handle) left ----
        const size_t rec = pair * (size_t)A.horizon + (size_t)it;   // this step's row in actions_out / obs_out
        if (Q.obs_out != nullptr && alive)
            for (int i = b; i < OD; i += L) Q.obs_out[rec * (size_t)OD + i] = row[i];
        const float a = Q.hidden == 64 ? policy_forward<64, L, AD>(lds, m, Q, OD, b, g) : policy_forward<32, L, AD>(lds, m, Q, OD, b, g);
        if (b < AD) {
            oa[b] = a;
            if (Q.actions_out != nullptr && alive) Q.actions_out[rec * (size_t)AD + b] = a;
        }
        wave_sync();
        if (commands) {
#pragma unroll
            for (int i = 0; i < AD; ++i) act[i] = oa[i];
        }

        is_robot = alive && b < N; is_ball = alive && b == N;
        const float obs_ts = prev_pot;   // the task scalar as this step's observation sees it (before the reward moves it)
        const bool first_step = steps == 0;
        const uint32_t t = tick0 + (uint32_t)it;
        if (is_ball && first_step) {
#pragma unroll
            for (int i = 0; i < 10; ++i) info[i] = 0.0f;
        }
        const float lastx = o.x, lasty = o.y;

        // ---- actions -> commands ----
        float q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const StepDraw dr = draw_for_step<KIND, TASK>(P, env_id, t, b, is_robot, fed);
#include "rsx_step_commands.inc"

        // ---- physics ----
        physics<KIND, L, NR>(P, o, b, g, alive, sh, cf);

        // ---- wire-format values, the observation the next step's action answers, reward ----
#include "rsx_step_wire.inc"
        write_obs<KIND, TASK>(P, row, b, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd, o.ir, obs_ts);
#include "rsx_step_xr.inc"
        wave_sync();
        float reward = 0.0f; int term = 0;
        if (is_ball) {
            bool success = false, against = false;
            task_reward<KIND, TASK>(P, sh.x0[g], o.x, o.y, lastx, lasty, first_step, prev_pot, info, reward, term, success, against);
        }
        if (alive) steps += 1;
        const int trunc = steps >= P.max_steps;
        // ret = ret + disc * reward; disc = disc * gamma — in this order, f32 (lanes other than the ball's add zeros)
        ret = alive ? ret + disc * reward : ret;
        disc = disc * A.gamma;
        n_sim = alive ? it + 1 : n_sim;
        const unsigned long long endm = __ballot(is_ball && (term | trunc));
        const bool ended = alive && ((endm >> (LaneMap<L>::slot(N, g))) & 1ull) != 0;
        if (is_ball && ended) fl = term | (trunc << 1);

        // ---- the pair's last simulated step: its observation (the terminal one if the episode ended) ----
        const bool last = ended || (alive && it + 1 == horizon);
        if (RSX_RARE_B(KIND, 4, __any(last))) {
            if (last && last_obs != nullptr)
                write_obs<KIND, TASK>(P, last_obs + pair * (size_t)OD, b, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd, o.ir, obs_ts);
            if (ended) {   // the pair idles from here on: its lanes hold zeros like the idle lanes of a tile
                alive = false;
                o = Body{};
            }
        }
        wave_sync();
    }

    if (live && b == N) {
        returns[pair] = ret;
        steps_out[pair] = n_sim;
        flags_out[pair] = (uint8_t)fl;
    }
}

template <int L>
size_t static_lds() { return sizeof(Shared<L>); }

template <bool PHYS>
void policy_launch(const Params& P, const int L, const int NR, const float* phys, const PlanArgs& A, const PolicyArgs& Q, const int act_dim,
                   float* returns, int32_t* steps, uint8_t* flags, float* last_obs, hipStream_t s) {
    const int grid = lane_grid(L, P.num_envs) * A.n_cand;   // (checked by the caller: fits the launch limit)
    with_task(P.task, [&](auto kind, auto task, auto nrs, auto fixed) {
        if constexpr (task != RSX_TASK_SSL_SCRIMMAGE) {   // (the scrimmage commands every robot: refused by the caller)
            with_task_variant<task, nrs, fixed, 32>(L, NR, [&](auto l, auto nr) {   // (64 lanes per env: refused by the caller)
                const size_t lds = sizeof(float) * (size_t)policy_image(64 / l, P.obs_dim, act_dim, Q.layers, Q.hidden).total;
                rsx_launch((task_lookahead_policy_kernel<kind, task, l, nr, PHYS>), dim3((unsigned)grid), dim3(64), lds, s, returns, steps, flags,
                           last_obs, grid >> 3, P, A, Q, phys);
            });
        }
    });
}

}  // namespace

long long policy_lds_bytes(const int L, const int obs_dim, const int act_dim, const PolicySpec& p) {
    const size_t fixed = L == 8 ? static_lds<8>() : L == 16 ? static_lds<16>() : static_lds<32>();
    return (long long)fixed + 4ll * (long long)policy_image(64 / L, obs_dim, act_dim, p.layers, p.hidden).total;
}

void launch_task_lookahead_policy(const Params& P, const int L, const int NR, const float* state, const float* aux, const float* obs,
                                  const uint32_t* ticks, const float* phys, const PolicySpec& p, const float* params, const int n_params,
                                  const int act_dim, const int n_policies, const int horizon, const float gamma, float* returns, int32_t* steps,
                                  uint8_t* flags, float* last_obs, float* actions_out, float* obs_out, hipStream_t s) {
    const PlanArgs A{state, aux, ticks, n_policies, horizon, gamma};
    const PolicyArgs Q{params, obs, actions_out, obs_out, n_params, p.layers, p.hidden, p.hidden_act, p.out_act};
    if (phys) policy_launch<true>(P, L, NR, phys, A, Q, act_dim, returns, steps, flags, last_obs, s);
    else policy_launch<false>(P, L, NR, nullptr, A, Q, act_dim, returns, steps, flags, last_obs, s);
}

}  // namespace rsx
