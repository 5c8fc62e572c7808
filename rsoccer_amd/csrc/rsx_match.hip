// rsx_match.hip — policy-vs-policy matches of VSS-v0 inside the lookahead launch (include/rsx.h: rsx_task_lookahead_match), in a
// translation unit of its own so that the instantiations of every existing kernel stay exactly what they were.
//
// task_lookahead_match_kernel is the loop of task_lookahead_policy_kernel (rsx_policy.hip) — load once, `alive`, stop at the env's first
// episode end, no store to the handle — with what task_collect_team_kernel (rsx_teamplay.hip) adds to the collector: a second policy
// image in LDS, the mirrored row next to every write_obs of the agent's row, the in-place seat exchange around each seat's forward, and
// the commands of every seated robot but blue 0 replaced behind rsx_step_commands.inc.  Triple (env e, actor k, opponent m) is played
// from where env e stands now; the heads are deterministic (sample = mean, action = out_act(mean)), so with the same parameters the
// rows before a pair's end are rsx_task_collect_team's rows bit for bit: both build the step from the same pieces and text fragments.
//
// Grid: one 64-lane workgroup per (tile, k, m), runs of K * M consecutive workgroups per tile (rsx_plan.hip's mapping with K * M
// candidates): v = tile_of_block, tile = v / (K M), k = (v % (K M)) / M, m = v % M.  The workgroup stages row k of the actor's parameters
// and row m of the opponent's.
// LDS per workgroup: Shared<L> + one image per side, an image being rsx_policy_mlp.hpp's with the team unit's action slot of
// max(8, round4(2 n_blue)) floats per env.  VSS-v0 3v3 at 8 lanes per env, 40-64-64-2 on both sides: 2 x 36 384 B + 6 272 B static =
// 79 040 B, what self-play takes — TWO workgroups per CU of the 163 840 B.  5v5 at 16 lanes per env (64-64-64-2 twice): 84 736 B, ONE
// workgroup per CU.  More than 64 KB of dynamic LDS: the launch raises the kernel's limit first (match_launch); the host refuses
// images beyond a CU's 160 KB.
//
// Memory traffic of the loop: stores only.  Every load — both policies' weights, state, scalars, the observation row — is issued ahead
// of the loop and lands behind ONE vmcnt(0).
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

struct MatchArgs {         // pair p = (e * K + k) * M + m; H = horizon, S / S2 = the sides' seat counts
    float* returns;        // [B][K][M]
    int32_t* steps;        // [B][K][M]
    uint8_t* flags;        // [B][K][M] bit 0 terminated, bit 1 truncated
    int8_t* result;        // [B][K][M] or nullptr
    float* last_obs;       // [B][K][M][obs_dim] or nullptr
    int n_opp;             // M (K * M is PlanArgs::n_cand)
};

struct MatchSide {         // one side's record and seat count (its policies travel in PolicyArgs)
    float* obs;            // [B][K][M][H][S][obs_dim] or nullptr
    float* actions;        // [B][K][M][H][S][2] or nullptr
    int seats;             // S
};

template <int KIND, int TASK, int L, int NR, bool PHYS>
__global__ __launch_bounds__(64) void task_lookahead_match_kernel(const int per_xcd, const Params P, const PlanArgs A, const PolicyArgs Q,
                                                                  const PolicyArgs Q2, const MatchArgs C, const MatchSide SA_, const MatchSide SO_,
                                                                  const float* __restrict__ phys) {
    using K = KC<KIND>;
    using T = TC<TASK>;
    constexpr int G = 64 / L;
    constexpr int ID = T::info_dim;
    constexpr int AD = T::act_dim;
    static_assert(KIND == RSX_KIND_VSS && TASK == RSX_TASK_VSS_V0 && AD == 2 && AD <= L && L >= 8, "VSS-v0 only: a seat takes two wheel commands");
    __shared__ Shared<L> sh;
    extern __shared__ float4 policy_lds4[];
    float* const lds = reinterpret_cast<float*>(policy_lds4);
#ifdef RSX_TIMING
    if (threadIdx.x == 0) sh.dbg = nullptr;
#endif
    const int lane = threadIdx.x;
    const int b = LaneMap<L>::body(lane), g = LaneMap<L>::env(lane);
    // (tile, actor, opponent) of this workgroup: rsx_plan.hip's mapping with K * M candidates per tile
    const int v = tile_of_block(per_xcd);
    const int tile = v / A.n_cand, km = v - tile * A.n_cand;
    const int k = km / C.n_opp, m_ix = km - k * C.n_opp;
    const int e = tile * G + g;
    const int N = NR ? NR : P.n_robots;
    const int NB = NR ? NR / 2 : P.n_blue;   // equal teams (checked by the host)
    const bool live = e < P.num_envs;
    const uint32_t env_id = P.env_id_base + (uint32_t)e;
    constexpr int OD_C = obs_dim_c<TASK, NR>();
    const int OD = OD_C ? OD_C : P.obs_dim;
    const int SA = SA_.seats, SO = SO_.seats;   // (uniform: launch arguments, checked by the host)
#define auxe(ROW) at_byte(A.aux, (ix_t)(ROW) * ((ix_t)4 * (ix_t)P.row_stride) + (ix_t)4 * (ix_t)e)   // row ROW of this env in the scalar arena
    const size_t pair = (size_t)e * (size_t)A.n_cand + (size_t)km;   // row of this pair in every output

    // ---- both policies' weights -> LDS, once; the env's current observation -> its row ----
    const int AP = action_pitch(NB);
    const PolicyImage m = policy_image(G, OD, AD, Q.layers, Q.hidden);
    const PolicyImage m2 = policy_image(G, OD, AD, Q2.layers, Q2.hidden);
    float* const lds2 = lds + image_floats(m, G, AP);   // (a multiple of 4 floats: the second image is 16-byte aligned like the first)
    stage_policy(Q.params + (size_t)k * (size_t)Q.n_params, lds, m, Q, OD, AD, lane);
    stage_policy(Q2.params + (size_t)m_ix * (size_t)Q2.n_params, lds2, m2, Q2, OD, AD, lane);
    float* const row = lds + m.rows + g * m.xs;                   // this env's observation
    float* const oa = lds + m.rows + 3 * G * m.xs + g * AP;       // ... and the actions the actor's seats answer with
    float* const row2 = lds2 + m2.rows + g * m2.xs;               // the mirrored observation
    float* const oa2 = lds2 + m2.rows + 3 * G * m2.xs + g * AP;   // ... and the opponent's answers
    for (int i = b; i < OD; i += L) {
        row[i] = live ? Q.obs[(size_t)e * OD + i] : 0.0f;
        if (!live) row2[i] = 0.0f;
    }

    // ---- load: the env's state and task scalars, once (as rsx_policy.hip) ----
    bool is_robot = live && b < N, is_ball = live && b == N;
    Body o; float od, wd, wheels[4];
    const RawBody raw = load_raw<KIND>(P, A.state, e, b, is_robot, is_ball);
    std::conditional_t<PHYS, EnvCoef, LitCoef<KIND>> cf{};
    if constexpr (PHYS) if (live) load_coefs(P, phys, e, cf);
    int steps = 0;
    if (live) steps = __float_as_int(auxe(ROW_STEPS));
    float ou0 = 0.0f, ou1 = 0.0f;
    if (is_robot && b >= 1) {
        ou0 = auxe(ROW_OU + 2 * b); ou1 = auxe(ROW_OU + 2 * b + 1);
    }
    float info[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    float prev_pot = 0.0f;
    if (is_ball) {
#pragma unroll
        for (int i = 0; i < ID; ++i)
            if (!(i == 0 || i >= 4)) info[i] = auxe(ROW_INFO + i);   // (VSS-v0: the terms a step carries over; the task scalar is derived below)
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
    // where this lane's robot finds its seat's two outputs (nullptr: not seated, or blue 0, whose action takes the `fed` path)
    const float* seat_act = nullptr;
    if (is_robot && b >= 1 && b < SA) seat_act = oa + 2 * b;
    if (is_robot && b >= NB && b - NB < SO) seat_act = oa2 + 2 * (b - NB);
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

    // per-pair results, held by every lane of the pair (the ball lane's copy is the one that counts)
    float ret = 0.0f, disc = 1.0f;
    int n_sim = 0, fl = 0, res = 0;
    bool alive = live;   // the pair's env has not ended yet
    wave_sync();         // weights and rows are in place

    for (int it = 0; it < horizon; ++it) {
        if (!__any(alive)) break;   // every env of the wave has ended (or the tile holds none)
        const size_t rec = pair * (size_t)A.horizon + (size_t)it;   // this step's row of this pair in every record
        // ---- every seat's a_t = out_act(policy(seat row of obs_t)): all of them answer the rows the previous step (or the handle) left ----
#pragma nounroll
        for (int j = 0; j < SA + SO; ++j) {
            const bool opp = j >= SA;   // (uniform) the actor's seats first, then the opponent's
            const int s = opp ? j - SA : j, S = opp ? SO : SA;
            const PolicyArgs Qj = opp ? Q2 : Q;
            // (selected value by value: a reference to the chosen side would be read back from the kernel arguments inside the loop)
            float* const x_obs = opp ? SO_.obs : SA_.obs;
            float* const x_actions = opp ? SO_.actions : SA_.actions;
            float* const ldj = opp ? lds2 : lds;
            float* const rj = opp ? row2 : row;
            float* const oj = opp ? oa2 : oa;
            const PolicyImage mj = policy_image(G, OD, AD, Qj.layers, Qj.hidden);
            const size_t srec = rec * (size_t)S + (size_t)s;   // this step's row of this (pair, seat)
            if (s > 0) {
                exchange_own(rj, s, b);
                wave_sync();
            }
            if (alive && x_obs != nullptr)   // recorded from the LDS row the policy reads: the recorded bits are the bits it saw
                for (int i = b; i < OD; i += L) x_obs[srec * (size_t)OD + i] = rj[i];
            const float a = Qj.hidden == 64 ? policy_forward<64, L, AD>(ldj, mj, Qj, OD, b, g) : policy_forward<32, L, AD>(ldj, mj, Qj, OD, b, g);
            if (s > 0) exchange_own(rj, s, b);   // back (the first layer, the row's only reader, is behind policy_forward's wave_sync)
            if (b < AD) {
                oj[2 * s + b] = a;
                if (alive && x_actions != nullptr) x_actions[srec * (size_t)AD + b] = a;
            }
            wave_sync();
        }
        if (commands) {
#pragma unroll
            for (int i = 0; i < AD; ++i) act[i] = oa[i];
        }

        is_robot = alive && b < N; is_ball = alive && b == N;
        const float obs_ts = prev_pot;   // the task scalar as this step's observation sees it (before the reward moves it)
        const bool first_step = steps == 0;
        const uint32_t t = tick0 + (uint32_t)it;   // the env's real future draws: keyed by the handle's step count
        if (is_ball && first_step) {
#pragma unroll
            for (int i = 0; i < 10; ++i) info[i] = 0.0f;
        }
        const float lastx = o.x, lasty = o.y;

        // ---- actions -> commands; a seated robot's is its seat's (its OU state has advanced in the fragment, unused) ----
        float q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const StepDraw dr = draw_for_step<KIND, TASK>(P, env_id, t, b, is_robot, fed);
#include "rsx_step_commands.inc"
        if (is_robot && seat_act != nullptr) {
            q[0] = vss_wheel(seat_act[0]); q[1] = vss_wheel(seat_act[1]);
            robot_targets<KIND>(P, o, q);
        }

        // ---- physics ----
        physics<KIND, L, NR>(P, o, b, g, alive, sh, cf);

        // ---- wire-format values, the observations the next step's actions answer, reward ----
#include "rsx_step_wire.inc"
        write_obs<KIND, TASK>(P, row, b, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd, o.ir, obs_ts);
        write_obs_mirrored(P, row2, b, NB, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd);
#include "rsx_step_xr.inc"
        wave_sync();
        float reward = 0.0f; int term = 0;
        bool success = false, against = false;   // the step ended on a goal for blue / against it
        if (is_ball) task_reward<KIND, TASK>(P, sh.x0[g], o.x, o.y, lastx, lasty, first_step, prev_pot, info, reward, term, success, against);
        if (alive) steps += 1;
        const int trunc = steps >= P.max_steps;
        // ret = ret + disc * reward; disc = disc * gamma — in this order, f32 (lanes other than the ball's add zeros)
        ret = alive ? ret + disc * reward : ret;
        disc = disc * A.gamma;
        n_sim = alive ? it + 1 : n_sim;
        const unsigned long long endm = __ballot(is_ball && (term | trunc));
        const bool ended = alive && ((endm >> (LaneMap<L>::slot(N, g))) & 1ull) != 0;
        if (is_ball && ended) {
            fl = term | (trunc << 1);
            // VSS-v0's task_reward reports a goal in the info terms the metrics count (rsx_step_vss_metrics.inc: info[4] goals for,
            // info[5] against) and leaves `success` / `against` as they were; zero until the step that ends the pair
            res = (success || info[4] > 0.0f) ? 1 : (against || info[5] > 0.0f) ? -1 : 0;
        }

        // ---- the pair's last simulated step: its observation (the terminal one if the episode ended) ----
        const bool last = ended || (alive && it + 1 == horizon);
        if (RSX_RARE_B(KIND, 4, __any(last))) {
            if (last && C.last_obs != nullptr)
                write_obs<KIND, TASK>(P, C.last_obs + pair * (size_t)OD, b, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd, o.ir, obs_ts);
            if (ended) {   // the pair idles from here on: its lanes hold zeros like the idle lanes of a tile
                alive = false;
                o = Body{};
            }
        }
        wave_sync();
    }

    if (live && b == N) {
        C.returns[pair] = ret;
        C.steps[pair] = n_sim;
        C.flags[pair] = (uint8_t)fl;
        if (C.result != nullptr) C.result[pair] = (int8_t)res;
    }
}

template <int L> constexpr size_t static_lds() { return sizeof(Shared<L>); }

// dynamic LDS of one workgroup: the actor's image and the opponent's behind it
size_t images_bytes(const int L, const int obs_dim, const int act_dim, const int n_blue, const PolicySpec& a, const PolicySpec& o) {
    const int G = 64 / L, AP = action_pitch(n_blue);
    return sizeof(float) * ((size_t)image_floats(policy_image(G, obs_dim, act_dim, a.layers, a.hidden), G, AP) +
                            (size_t)image_floats(policy_image(G, obs_dim, act_dim, o.layers, o.hidden), G, AP));
}

template <bool PHYS>
void match_launch(const Params& P, const int L, const int NR, const float* phys, const PlanArgs& A, const PolicyArgs& Q, const PolicyArgs& Q2,
                  const MatchArgs& C, const MatchSide& SA, const MatchSide& SO, const size_t lds, hipStream_t s) {
    const int grid = lane_grid(L, P.num_envs) * A.n_cand;   // (checked by the caller: fits the launch limit)
    with_task_variant<RSX_TASK_VSS_V0, 6, false, 32>(L, NR, [&](auto l, auto nr) {   // (64 lanes per env: refused by the caller)
        const auto kernel = task_lookahead_match_kernel<RSX_KIND_VSS, RSX_TASK_VSS_V0, l, nr, PHYS>;
        // dynamic LDS beyond 64 KB is the kernel's to be granted first: once per variant and device, and again for a larger image
        static std::atomic<int> granted[64];
        int dev = 0;
        if (lds > 65536 && hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 && granted[dev].load(std::memory_order_relaxed) < (int)lds) {
            const hipError_t rc = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (rc == hipSuccess) granted[dev].store((int)lds, std::memory_order_relaxed);
            else if (g_launch_status == hipSuccess) g_launch_status = rc;
        }
        rsx_launch(kernel, dim3((unsigned)grid), dim3(64), lds, s, grid >> 3, P, A, Q, Q2, C, SA, SO, phys);
    });
}

}  // namespace

long long match_lds_bytes(const int L, const int obs_dim, const int act_dim, const int n_blue, const PolicySpec& actor, const PolicySpec& opponent) {
    const size_t fixed = L == 8 ? static_lds<8>() : L == 16 ? static_lds<16>() : static_lds<32>();
    return (long long)fixed + (long long)images_bytes(L, obs_dim, act_dim, n_blue, actor, opponent);
}

void launch_task_lookahead_match(const Params& P, const int L, const int NR, const float* state, const float* aux, const float* obs,
                                 const uint32_t* ticks, const float* phys, const PolicySpec& p, const float* params, const int n_params,
                                 const int n_actors, const int seats, const PolicySpec& opp, const float* opp_params, const int n_opp_params,
                                 const int n_opponents, const int opp_seats, const int act_dim, const int horizon, const float gamma,
                                 const rsx_match_out& out, hipStream_t s) {
    const PlanArgs A{state, aux, ticks, n_actors * n_opponents, horizon, gamma};
    const PolicyArgs Q{params, obs, nullptr, nullptr, n_params, p.layers, p.hidden, p.hidden_act, p.out_act};
    // (the opponent's row is the mirror of the state, computed in the kernel: it reads no obs buffer)
    const PolicyArgs Q2{opp_params, nullptr, nullptr, nullptr, n_opp_params, opp.layers, opp.hidden, opp.hidden_act, opp.out_act};
    const MatchArgs C{out.returns, out.steps, out.flags, out.result, out.last_obs, n_opponents};
    const MatchSide SA{out.obs, out.actions, seats}, SO{out.opp_obs, out.opp_actions, opp_seats};
    const size_t lds = images_bytes(L, P.obs_dim, act_dim, P.n_blue, p, opp);
    if (phys) match_launch<true>(P, L, NR, phys, A, Q, Q2, C, SA, SO, lds, s);
    else match_launch<false>(P, L, NR, nullptr, A, Q, Q2, C, SA, SO, lds, s);
}

}  // namespace rsx
