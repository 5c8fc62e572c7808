// rsx_plan_body.inc — the per-pair loop of the lookahead kernels (rsx_plan.hip: task_lookahead_kernel, rsx_plan_sampled.hip:
// task_lookahead_sampled_kernel), included as the kernel's body the way rsx_task_step_body.inc is; the pieces of a step that
// both state (rsx_step_commands.inc, rsx_step_wire.inc, rsx_step_xr.inc) are included by both.  The including kernel names
// KIND, TASK, L, NR and PHYS as template parameters and returns, steps_out, flags_out, last_obs, per_xcd, P, A (PlanArgs) and phys as
// arguments.  Where a step's action comes from is the includer's: two macros, expanded inside the body's scope (e, b, k, pair, N,
// AD, step_floats, tick0, A are visible):
//   RSX_PLAN_ACT_SETUP             declarations in front of the first fetch
//   RSX_PLAN_ACT_FETCH(DST, STEP)  DST[0 .. AD) := the action of step STEP of this pair's commanding lane (only those lanes run it)
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
    constexpr int OD_C = obs_dim_c<TASK, NR>();
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
    // the candidate's actions, act_dim floats per commanding lane and step; the scrimmage commands every robot (a step holds
    // N * act_dim floats there)
    const bool commands = TASK == RSX_TASK_SSL_SCRIMMAGE ? is_robot : (is_robot && b == 0);
    const size_t step_floats = TASK == RSX_TASK_SSL_SCRIMMAGE ? (size_t)N * AD : (size_t)AD;
    constexpr bool fed = true;   // every step's action is a candidate's: the shared fragments and draw_for_step never draw the agent's
    RSX_PLAN_ACT_SETUP
    float act[AD];
#pragma unroll
    for (int i = 0; i < AD; ++i) act[i] = 0.0f;
    if (commands && horizon > 0) {
        RSX_PLAN_ACT_FETCH(act, 0)
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
            RSX_PLAN_ACT_FETCH(act_next, it + 1)
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

        // ---- wire-format values, reward ----
#include "rsx_step_wire.inc"
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
#pragma unroll
        for (int i = 0; i < AD; ++i) act[i] = act_next[i];
        wave_sync();
    }

    if (live && b == N) {
        returns[pair] = ret;
        steps_out[pair] = n_sim;
        flags_out[pair] = (uint8_t)fl;
    }
