// rsx_plan.hip — exact lookahead over candidate action sequences (include/rsx.h: rsx_task_lookahead), in a translation unit of
// its own so that the instantiations of every existing kernel stay exactly what they were.
//
// task_lookahead_kernel runs, per (env, candidate) pair, up to `horizon` fused task steps from the env's CURRENT state with the
// candidate's actions in place of the fed action and the handle's real per-step draws (OU noise of the other robots) for the ticks
// the handle would take next, all in registers, and sums the discounted rewards.  It reads the handle's buffers and writes only
// its own outputs: the handle is left exactly as it was.
//
// The body is the `mode == 0` branch of rsx_task_step_body.inc built from the same device functions (load_raw, interpret_body,
// draw_for_step, vss_wheel, ssl_agent_commands, robot_targets, physics, wheel_speeds, write_obs, task_reward), the way
// trace_eval_phys_kernel (rsx_sysid.hip) was built from the raw step: between two steps the lane's record goes through the same
// wire-format round trip (heading in degrees, rate through deg/s, sin / cos re-derived from the stored heading, ball height through
// r_ball + z) that a store and a reload apply, so a pair's rewards, flags and observations are bit for bit those of `horizon`
// rsx_task_step calls with the candidate's actions.  What the step body does at an episode end — placement, auto-reset, physics
// redraw, metrics — is NOT simulated: a pair stops at its env's first episode end.
//
// Grid: one lane group per pair, tiles(num_envs) x K workgroups.  Workgroup -> (tile, candidate): the XCD's share of the grid is
// cut into runs of K consecutive workgroups that hold the K candidates of ONE tile, so the state rows of a tile are fetched from
// HBM once per XCD and the other K - 1 groups find them in that XCD's L2.
//
// Registers: the per-pair accumulators (return, discount, step count, flags) are plain scalars held by every lane and advanced
// through selects — indexed by role they would go to scratch memory (see the note on Acc in rsx_sysid.hip).  The observation is
// written once per pair (at its end or after the last step), not per step.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rsx.h"
#include "rsx_units.hpp"
#include "rsx_variants.hpp"

namespace rsx {

namespace {

struct PlanArgs {
    const float* state;      // the handle's state rows (read only)
    const float* aux;        // the handle's scalar arena (read only)
    const uint32_t* ticks;   // device-keyed handles: the step-counter slots (slot 0 is read, never written), else nullptr
    int n_cand, horizon;
    float gamma;
};

template <int KIND, int TASK, int L, int NR, bool PHYS>
__global__ __launch_bounds__(64) void task_lookahead_kernel(const float* __restrict__ actions, float* __restrict__ returns,
                                                            int32_t* __restrict__ steps_out, uint8_t* __restrict__ flags_out,
                                                            float* __restrict__ last_obs, const int per_xcd, const Params P,
                                                            const PlanArgs A, const float* __restrict__ phys) {
    using K = KC<KIND>;
    using T = TC<TASK>;
    constexpr int G = 64 / L;
    constexpr int ID = T::info_dim;
    constexpr int AD = T::act_dim;
    __shared__ Shared<L> sh;
#ifdef RSX_TIMING
    if (threadIdx.x == 0) sh.dbg = nullptr;
#endif
    const int lane = threadIdx.x;
    const int b = LaneMap<L>::body(lane), g = LaneMap<L>::env(lane);
    // (tile, candidate) of this workgroup: see the header
    const int v = tile_of_block(per_xcd);
    const int tile = v / A.n_cand, k = v - tile * A.n_cand;
    const int e = tile * G + g;
    const int N = NR ? NR : P.n_robots;
    const bool live = e < P.num_envs;
    const uint32_t env_id = P.env_id_base + (uint32_t)e;
    constexpr int OD_C = NR == 0 ? 0
        : TASK == RSX_TASK_VSS_V0 ? 4 + 6 * NR
        : TASK == RSX_TASK_SSL_STATIC_DEFENDERS ? 4 + 8 + 2 * (NR - 1)
        : TASK == RSX_TASK_SSL_SCRIMMAGE ? 2 + 2 * NR
        : TASK == RSX_TASK_SSL_DRIBBLING ? 21 : TASK == RSX_TASK_SSL_CONTESTED ? 14 : 16;
    const int OD = OD_C ? OD_C : P.obs_dim;
#define auxe(ROW) at_byte(A.aux, (ix_t)(ROW) * ((ix_t)4 * (ix_t)P.row_stride) + (ix_t)4 * (ix_t)e)   // row ROW of this env in the scalar arena
    const size_t pair = (size_t)e * (size_t)A.n_cand + (size_t)k;   // row of this pair in every output

    // ---- load: the env's state and task scalars, once ----
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
    // the handle's step counter, not advanced: the host's count, or slot 0 of a device-keyed handle (all slots hold the same value
    // between launches).  A counter that `horizon` more steps would wrap: nothing is simulated (every pair reports 0 steps)
    uint32_t tick0 = P.tick_base;
    int horizon = A.horizon;
    if (A.ticks != nullptr) {
        tick0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.ticks[0]);
        if (tick0 > 0xFFFFFFFFu - (uint32_t)horizon) horizon = 0;
    }
    // the candidate's actions: [num_envs][K][H][act_dim]; the scrimmage commands every robot (act_dim floats per robot and step)
    const bool commands = TASK == RSX_TASK_SSL_SCRIMMAGE ? is_robot : (is_robot && b == 0);
    const size_t step_floats = TASK == RSX_TASK_SSL_SCRIMMAGE ? (size_t)N * AD : (size_t)AD;
    const float* const my_act = actions + pair * (size_t)A.horizon * step_floats + (TASK == RSX_TASK_SSL_SCRIMMAGE ? (size_t)b * AD : 0);
    float act[AD];
#pragma unroll
    for (int i = 0; i < AD; ++i) act[i] = 0.0f;
    if (commands && horizon > 0) {
#pragma unroll
        for (int i = 0; i < AD; ++i) act[i] = my_act[i];
    }
    interpret_body<KIND>(raw, is_robot, is_ball, o, od, wd, wheels);
    if (TASK == RSX_TASK_VSS_V0 && is_ball) {
        // VSS-v0: the previous ball potential (vss_gym.py:256-283) is the potential of the ball where the step finds it — the same
        // expression on the same floats as task_reward's.  The one-lane-per-env step kernels recompute it the same way and do NOT keep
        // ROW_PREV_POT up to date (rsx_epl.hpp; rsx_task_checkpoint_save patches the row for the same reason), so the row is not read
        // here on any layout.  (The first step of an episode ignores the value.)
        prev_pot = vss_ball_potential(o.x, o.y, P.hl_goal, P.inv_len_cm);
    }

    // per-pair results, held by every lane of the pair (the ball lane's copy is the one that counts)
    float ret = 0.0f, disc = 1.0f;
    int n_sim = 0, fl = 0;
    bool alive = live;   // the pair's env has not ended yet

    for (int it = 0; it < horizon; ++it) {
        if (!__any(alive)) break;   // every env of the wave has ended (or the tile holds none)
        // the next step's actions travel while this step computes
        float act_next[AD];
#pragma unroll
        for (int i = 0; i < AD; ++i) act_next[i] = 0.0f;
        if (commands && alive && it + 1 < horizon) {
#pragma unroll
            for (int i = 0; i < AD; ++i) act_next[i] = my_act[(size_t)(it + 1) * step_floats + i];
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
        const StepDraw dr = draw_for_step<KIND, TASK>(P, env_id, t, b, is_robot, true);
        if (TASK == RSX_TASK_VSS_V0) {
            if (is_robot) {
                float a0, a1;
                if (b == 0) { a0 = act[0]; a1 = act[1]; }
                else {
                    ou0 = (ou0 + P.ou_theta_dt * (0.0f - ou0)) + P.ou_sig_sqdt * dr.v[0];
                    ou1 = (ou1 + P.ou_theta_dt * (0.0f - ou1)) + P.ou_sig_sqdt * dr.v[1];
                    a0 = ou0; a1 = ou1;
                }
                q[0] = vss_wheel(a0); q[1] = vss_wheel(a1);
            }
        } else if (TASK == RSX_TASK_SSL_SCRIMMAGE) {
            if (is_robot) {
                q[1] = act[0] * T::max_v; q[2] = act[1] * T::max_v; q[3] = act[2] * 10.0f;
                q[5] = act[3] > 0.9f ? 5.0f : 0.0f;
            }
        } else {
            if (is_robot && b == 0) {
                float a[5] = {0, 0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < AD; ++i) a[i] = act[i];
                ssl_agent_commands<TASK>(a, o.s, o.c, q);
            }
            if (TASK == RSX_TASK_SSL_PASS_ENDURANCE && is_robot && b == 1) q[7] = 1.0f;
        }
        if (is_robot) robot_targets<KIND>(P, o, q);

        // ---- physics ----
        physics<KIND, L, NR>(P, o, b, g, alive, sh, cf);

        // ---- wire-format values, reward ----
        if (is_robot) {
            od = o.th; wd = o.om * K::rad2deg;
            if (KIND == RSX_KIND_SSL) wheel_speeds<KIND>(P, o, wheels);
            o.om = wd * K::deg2rad;
            sincos_f32(o.th * K::deg2rad, o.s, o.c);
        } else if (is_ball) {
            o.z = (K::r_ball + o.z) - K::r_ball;
        }
        if (is_robot && b == 0) {
            float* xr = sh.x0[g];
            xr[0] = o.x; xr[1] = o.y;
            if (TASK == RSX_TASK_VSS_V0) { xr[2] = o.vx; xr[3] = o.vy; xr[4] = q[0]; xr[5] = q[1]; }
            else if (TASK == RSX_TASK_SSL_STATIC_DEFENDERS || TASK == RSX_TASK_SSL_CONTESTED) {
                xr[6] = lastx; xr[7] = lasty;
                xr[8] = wheels[0]; xr[9] = wheels[1]; xr[10] = wheels[2]; xr[11] = wheels[3];
            }
        } else if (is_robot) {
            float* xr = sh.x0[g];
            if (TASK == RSX_TASK_SSL_DRIBBLING) xr[1 + b] = (fabsf(o.vx) > 0.05f || fabsf(o.vy) > 0.05f) ? 1.0f : 0.0f;
            if (TASK == RSX_TASK_SSL_CONTESTED && b == 1) xr[2] = (fabsf(o.vx) > 0.1f || fabsf(o.vy) > 0.1f) ? 1.0f : 0.0f;
            if (TASK == RSX_TASK_SSL_PASS_ENDURANCE && b == 1) { xr[2] = o.x; xr[3] = o.y; xr[4] = o.ir ? 1.0f : 0.0f; }
        }
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
#pragma unroll
        for (int i = 0; i < AD; ++i) act[i] = act_next[i];
        wave_sync();
    }

    if (live && b == N) {
        returns[pair] = ret;
        steps_out[pair] = n_sim;
        flags_out[pair] = (uint8_t)fl;
    }
}

template <bool PHYS>
void plan_launch(const Params& P, const int L, const int NR, const float* phys, const PlanArgs& A, const float* actions, float* returns,
                 int32_t* steps, uint8_t* flags, float* last_obs, hipStream_t s) {
    const int grid = lane_grid(L, P.num_envs) * A.n_cand;   // (checked by the caller: fits the launch limit)
    with_task(P.task, [&](auto kind, auto task, auto nrs, auto fixed) {
        with_task_variant<task, nrs, fixed, 32>(L, NR, [&](auto l, auto nr) {   // (64 lanes per env: refused by rsx_task_lookahead)
            rsx_launch((task_lookahead_kernel<kind, task, l, nr, PHYS>), dim3((unsigned)grid), dim3(64), 0, s, actions, returns, steps, flags,
                       last_obs, grid >> 3, P, A, phys);
        });
    });
}

}  // namespace

long long lookahead_grid(const int L, const int num_envs, const int n_candidates) {
    return (long long)lane_grid(L, num_envs) * (long long)n_candidates;
}

void launch_task_lookahead(const Params& P, const int L, const int NR, const float* state, const float* aux, const uint32_t* ticks,
                           const float* phys, const float* actions, const int n_candidates, const int horizon, const float gamma,
                           float* returns, int32_t* steps, uint8_t* flags, float* last_obs, hipStream_t s) {
    const PlanArgs A{state, aux, ticks, n_candidates, horizon, gamma};
    if (phys) plan_launch<true>(P, L, NR, phys, A, actions, returns, steps, flags, last_obs, s);
    else plan_launch<false>(P, L, NR, nullptr, A, actions, returns, steps, flags, last_obs, s);
}

}  // namespace rsx
