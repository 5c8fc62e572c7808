// rsx_teamplay.hip — team play for VSS-v0: rsx_selfplay.hip's launch with EVERY robot of a side driven by that side's policy (include/rsx.h:
// rsx_task_collect_team).  A "seat" is a robot driven by a policy: blue seat i is blue robot i, yellow seat i is yellow robot i (body
// index n_blue + i).  All blue seats share the agent's parameters, all yellow seats the opponent's.  A translation unit of its own, a
// sibling of rsx_selfplay.hip and rsx_collect.hip, so that the instantiations of every existing kernel stay exactly what they were.
//
// task_collect_team_kernel follows the loop of task_collect_selfplay_kernel piece by piece (the same step pieces and text fragments, the
// same auto-reset) and differs in:
//   seat counts               run-time launch arguments: actor_seats in {1, n_blue}, opponent_seats in {0, 1, n_yellow}.  (1, 0) is the
//                             collector's launch, (1, 1) the self-play launch, bit for bit; without an opponent no second image is staged;
//   the seat's row            made IN PLACE: seat i's observation is the side's row with "own" slots 0 and i exchanged (7 floats at 4 + 7 k).
//                             Lanes 0 .. 6 of the env exchange the two slots in the env's LDS row, the forward runs, and the same lanes
//                             exchange them back — float moves, no arithmetic.  Seat rows side by side (6 x 8 x 68 floats) would cost
//                             13 056 B and the second workgroup per CU; the records are written through the same map (seat_ix);
//   one forward per seat      a run-time loop over the seats of both sides (#pragma nounroll: ONE inlined policy_forward per hidden
//                             width, not six), each seat's two outputs in floats 2 i, 2 i + 1 of the env's action slot;
//   the heads                 the agent's recipe with the seat index in Philox counter word 1: (env, seat, tick, dom | block << 8), dom 7
//                             for the agent and 9 for the opponent.  Seat 0 draws what the collector and self-play draw;
//   the commands              behind rsx_step_commands.inc the lane of every seated robot but blue 0 overwrites q[0], q[1] with vss_wheel
//                             of its seat's outputs and redoes robot_targets; blue 0 keeps the `fed` path.  Every Ornstein-Uhlenbeck
//                             state has advanced on its usual draws in the fragment, unused: the env can be handed back at any time.
// Reward, flags, metrics and the handle's obs / final_obs buffers stay the engine's (seat 0 of blue).
//
// Grid: the handle's lane-group grid (lane_grid), one 64-lane workgroup per tile.
// LDS per workgroup: Shared<L> + one image per side.  An image is rsx_policy_mlp.hpp's with an action slot of max(8, round4(2 n_blue))
// floats per env: 8 for 3v3 (three seats x 2), 12 for 5v5.  VSS-v0 3v3 at 8 lanes per env, 40-64-64-2 on both sides: 2 x 36 384 B +
// 6 272 B static = 79 040 B, what self-play takes — TWO workgroups per CU of the 163 840 B.  5v5 at 16 lanes per env (64-64-64-2 twice):
// 2 x 39 584 B + 5 568 B = 84 736 B, ONE workgroup per CU, as self-play.  Registers do not limit either (one wave per workgroup).  More
// than 64 KB of dynamic LDS: the launch raises the kernel's limit first (team_launch); the host refuses images beyond a CU's 160 KB.
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

// the opponent head's Philox domain word (rsx_selfplay.hip's; rsx_math.hpp: DOM_POLICY = 7; rsx_ppo_update.hip: DOM_PERM = 8)
constexpr uint32_t DOM_OPPONENT = 9u;

struct TeamArgs {
    float* rewards;        // [T][B]
    uint8_t* flags;        // [T][B] bit 0 terminated, bit 1 truncated
    uint32_t k0, k1;       // noise_seed lo, hi: the Philox key of every head's noise
};

struct SideArgs {          // one side's policy and record, S = seats
    const float* params;   // [P]
    const float* sigma;    // [2] or nullptr = deterministic
    float* obs;            // [T][B][S][obs_dim] or nullptr
    float* actions;        // [T][B][S][2] or nullptr
    float* mean;           // [T][B][S][2] or nullptr
    float* sample;         // [T][B][S][2] or nullptr
    float* final_obs;      // [T][B][S][obs_dim] or nullptr: rows of ended (t, env) only
    float* next_obs;       // [B][S][obs_dim] or nullptr
    int seats;             // S
};

// (the action slot and image sizes, the seat map seat_ix, the in-place exchange_own and the mirrored row write_obs_mirrored: rsx_seats.hpp)

// one component of a Gaussian head (rsx_selfplay.hip's, with the seat in counter word 1): component b takes normal b & 3 of block b >> 2
__device__ __forceinline__ float head_sample(const float mean, const float sigma, const uint32_t env_id, const uint32_t seat, const uint32_t t,
                                             const int b, const uint32_t dom, const uint32_t k0, const uint32_t k1) {
    const u32x4 u = philox4x32(env_id, seat, t, dom | ((uint32_t)(b >> 2) << 8), k0, k1);
    float n0, n1;
    plan_normal_pair((b & 2) ? u.z : u.x, (b & 2) ? u.w : u.y, n0, n1);
    const float eps = (b & 1) ? n1 : n0;
    return mean + sigma * eps;   // (two roundings: the unit is built with -ffp-contract=off)
}

// seat rows of one side -> a record: S rows of OD floats at dst, read from the side's LDS row through the seat map
__device__ __forceinline__ void store_seat_rows(float* __restrict__ dst, const float* row, const int S, const int OD, const int b, const int L) {
#pragma nounroll
    for (int s = 0; s < S; ++s)
        for (int i = b; i < OD; i += L) dst[(size_t)s * OD + i] = row[seat_ix(i, s)];
}

template <int KIND, int TASK, int L, int NR, bool PHYS>
__global__ __launch_bounds__(64) void task_collect_team_kernel(const int per_xcd, const int n_steps_arg, const Params P, const Buffers bufs,
                                                               const PolicyArgs Q, const PolicyArgs Q2, const TeamArgs C, const SideArgs A,
                                                               const SideArgs O, float* phys) {
    using K = KC<KIND>;
    using T = TC<TASK>;
    constexpr int G = 64 / L;
    constexpr int ID = T::info_dim;
    constexpr int AD = T::act_dim;
    constexpr int MODE = MODE_ROLLOUT;   // (what the shared fragments specialise on: the multi-step trip)
    constexpr int mode = 0;
    static_assert(KIND == RSX_KIND_VSS && TASK == RSX_TASK_VSS_V0 && AD == 2 && AD <= L && L >= 8, "VSS-v0 only: a seat takes two wheel commands");
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
    const int SA = A.seats, SO = O.seats;   // (uniform: launch arguments, checked by the host)
    const bool has_opp = SO > 0;
#define auxe(ROW) at_byte(bufs.aux, (ix_t)(ROW) * ((ix_t)4 * (ix_t)P.row_stride) + (ix_t)4 * (ix_t)e)   // row ROW of this env in the scalar arena

    // ---- both policies' weights -> LDS, once; the env's current observation -> its row; the heads' sigmas ----
    const int AP = action_pitch(NB);
    const PolicyImage m = policy_image(G, OD, AD, Q.layers, Q.hidden);
    float* const lds2 = lds + image_floats(m, G, AP);   // (a multiple of 4 floats: the second image is 16-byte aligned like the first)
    stage_policy(A.params, lds, m, Q, OD, AD, lane);
    float* const row = lds + m.rows + g * m.xs;                 // this env's observation
    float* const oa = lds + m.rows + 3 * G * m.xs + g * AP;     // ... and the actions the agent's seats answer with
    float* row2 = row;                                          // the mirrored observation and the opponent's answers (with an opponent)
    float* oa2 = oa;
    if (has_opp) {
        const PolicyImage m2 = policy_image(G, OD, AD, Q2.layers, Q2.hidden);
        stage_policy(O.params, lds2, m2, Q2, OD, AD, lane);
        row2 = lds2 + m2.rows + g * m2.xs;
        oa2 = lds2 + m2.rows + 3 * G * m2.xs + g * AP;
    }
    for (int i = b; i < OD; i += L) row[i] = live ? bufs.obs[(size_t)e * OD + i] : 0.0f;
    if (has_opp && !live)
        for (int i = b; i < OD; i += L) row2[i] = 0.0f;
    const bool noisy = A.sigma != nullptr, noisy2 = has_opp && O.sigma != nullptr;   // (uniform: launch arguments)
    float sigma = 0.0f, sigma2 = 0.0f;
    if (noisy && b < AD) sigma = A.sigma[b];
    if (noisy2 && b < AD) sigma2 = O.sigma[b];

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
    if (has_opp) write_obs_mirrored(P, row2, b, NB, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd);
    wave_sync();   // weights and rows are in place

    for (int it = 0; it < n_steps; ++it) {
        const uint32_t t = tick0 + (uint32_t)it;   // per-step draws are keyed by the handle's step count, not by the env's counters
        const size_t rec = (size_t)it * B + (size_t)e;   // this step's row of this env in every output
        // ---- every seat's a_t = head(policy(seat row of obs_t)): all of them answer the rows the previous step left ----
#pragma nounroll
        for (int k = 0; k < SA + SO; ++k) {
            const bool opp = k >= SA;   // (uniform) the agent's seats first, then the opponent's
            const int s = opp ? k - SA : k, S = opp ? SO : SA;
            const PolicyArgs Qk = opp ? Q2 : Q;
            // (selected value by value: a reference to the chosen side would be read back from the kernel arguments inside the loop)
            float* const x_obs = opp ? O.obs : A.obs;
            float* const x_actions = opp ? O.actions : A.actions;
            float* const x_mean = opp ? O.mean : A.mean;
            float* const x_sample = opp ? O.sample : A.sample;
            float* const ldk = opp ? lds2 : lds;
            float* const rk = opp ? row2 : row;
            float* const ok = opp ? oa2 : oa;
            const PolicyImage mk = policy_image(G, OD, AD, Qk.layers, Qk.hidden);
            const size_t srec = rec * (size_t)S + (size_t)s;   // this step's row of this (env, seat)
            if (s > 0) {
                exchange_own(rk, s, b);
                wave_sync();
            }
            if (live && x_obs != nullptr)   // recorded from the LDS row the policy reads: the recorded bits are the bits it saw
                for (int i = b; i < OD; i += L) x_obs[srec * (size_t)OD + i] = rk[i];
            const float mean = Qk.hidden == 64 ? policy_forward<64, L, AD, false>(ldk, mk, Qk, OD, b, g)
                                               : policy_forward<32, L, AD, false>(ldk, mk, Qk, OD, b, g);
            if (s > 0) exchange_own(rk, s, b);   // back (the first layer, the row's only reader, is behind policy_forward's wave_sync)
            if (b < AD) {
                const float smp = (opp ? noisy2 : noisy) ? head_sample(mean, opp ? sigma2 : sigma, env_id, (uint32_t)s, t, b,
                                                                        opp ? DOM_OPPONENT : DOM_POLICY, C.k0, C.k1)
                                                         : mean;
                const float a = policy_act(smp, Qk.out_act);
                ok[2 * s + b] = a;
                if (live) {
                    if (x_actions != nullptr) x_actions[srec * (size_t)AD + b] = a;
                    if (x_mean != nullptr) x_mean[srec * (size_t)AD + b] = mean;
                    if (x_sample != nullptr) x_sample[srec * (size_t)AD + b] = smp;
                }
            }
            wave_sync();
        }
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

        // ---- actions -> commands; a seated robot's is its seat's (its OU state has advanced in the fragment, unused) ----
        float q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const StepDraw dr = draw_for_step<KIND, TASK>(P, env_id, t, b, is_robot, fed);
#include "rsx_step_commands.inc"
        if (seat_act != nullptr) {
            q[0] = vss_wheel(seat_act[0]); q[1] = vss_wheel(seat_act[1]);
            robot_targets<KIND>(P, o, q);
        }

        // ---- physics ----
        physics<KIND, L, NR>(P, o, b, g, live, sh, cf);

        // ---- wire-format values, the observations the next step's actions answer, reward ----
#include "rsx_step_wire.inc"
        write_obs<KIND, TASK>(P, row, b, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd, o.ir, obs_ts);
        if (has_opp) write_obs_mirrored(P, row2, b, NB, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd);
#include "rsx_step_xr.inc"
        wave_sync();
#include "rsx_step_reward.inc"
        if (is_ball) {
            C.rewards[rec] = reward;
            C.flags[rec] = (uint8_t)(term | (trunc << 1));
        }

        // ---- episode end: same-step auto-reset ----
        if (RSX_RARE_B(KIND, 4, __any(ended))) {
            if (ended) {  // terminal observation: the handle's (seat 0's) from the registers, the seats' from the rows just written
                write_obs<KIND, TASK>(P, bufs.final_obs + (size_t)e * OD, b, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd, o.ir, obs_ts);
                if (A.final_obs != nullptr) store_seat_rows(A.final_obs + rec * (size_t)SA * (size_t)OD, row, SA, OD, b, L);
                if (has_opp && O.final_obs != nullptr) store_seat_rows(O.final_obs + rec * (size_t)SO * (size_t)OD, row2, SO, OD, b, L);
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
                if (has_opp) write_obs_mirrored(P, row2, b, NB, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd);
            }
            wave_sync();
        }

        wave_sync();
    }

    // ---- store: the state in wire format, the scalars, and the last observation into the handle's obs buffer ----
    store_body<KIND>(P, bufs.state, e, b, is_robot, is_ball, o, od, wd, wheels, P.n_sub != 0 || was_reset);
    if (live) {
        for (int i = b; i < OD; i += L) bufs.obs[(size_t)e * OD + i] = row[i];
        // ... and the seats' rows after the last step
        if (A.next_obs != nullptr) store_seat_rows(A.next_obs + (size_t)e * (size_t)SA * (size_t)OD, row, SA, OD, b, L);
        if (has_opp && O.next_obs != nullptr) store_seat_rows(O.next_obs + (size_t)e * (size_t)SO * (size_t)OD, row2, SO, OD, b, L);
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

// dynamic LDS of one workgroup: the agent's image and, with an opponent, the opponent's behind it
size_t images_bytes(const int L, const int obs_dim, const int act_dim, const int n_blue, const PolicySpec& a, const PolicySpec* o) {
    const int G = 64 / L, AP = action_pitch(n_blue);
    size_t n = (size_t)image_floats(policy_image(G, obs_dim, act_dim, a.layers, a.hidden), G, AP);
    if (o) n += (size_t)image_floats(policy_image(G, obs_dim, act_dim, o->layers, o->hidden), G, AP);
    return sizeof(float) * n;
}

template <bool PHYS>
void team_launch(const Params& P, const Buffers& b, const int L, const int NR, float* phys, const PolicyArgs& Q, const PolicyArgs& Q2,
                 const TeamArgs& C, const SideArgs& A, const SideArgs& O, const size_t lds, const int n_steps, hipStream_t s) {
    const int grid = lane_grid(L, P.num_envs);
    with_task_variant<RSX_TASK_VSS_V0, 6, false, 32>(L, NR, [&](auto l, auto nr) {   // (64 lanes per env: refused by the caller)
        const auto kernel = task_collect_team_kernel<RSX_KIND_VSS, RSX_TASK_VSS_V0, l, nr, PHYS>;
        // dynamic LDS beyond 64 KB is the kernel's to be granted first: once per variant and device, and again for a larger image
        static std::atomic<int> granted[64];
        int dev = 0;
        if (lds > 65536 && hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 && granted[dev].load(std::memory_order_relaxed) < (int)lds) {
            const hipError_t rc = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (rc == hipSuccess) granted[dev].store((int)lds, std::memory_order_relaxed);
            else if (g_launch_status == hipSuccess) g_launch_status = rc;
        }
        rsx_launch(kernel, dim3((unsigned)grid), dim3(64), lds, s, grid >> 3, n_steps, P, b, Q, Q2, C, A, O, phys);
    });
}

}  // namespace

long long team_lds_bytes(const int L, const int obs_dim, const int act_dim, const int n_blue, const PolicySpec& agent,
                         const PolicySpec* opponent) {
    const size_t fixed = L == 8 ? static_lds<8>() : L == 16 ? static_lds<16>() : static_lds<32>();
    return (long long)fixed + (long long)images_bytes(L, obs_dim, act_dim, n_blue, agent, opponent);
}

void launch_task_collect_team(const Params& P, const Buffers& b, const int L, const int NR, float* phys, const PolicySpec& p,
                              const float* params, const int n_params, const float* sigma, const int seats, const PolicySpec* opp,
                              const float* opp_params, const int n_opp_params, const float* opp_sigma, const int opp_seats,
                              const int act_dim, const uint64_t noise_seed, const int n_steps, const rsx_team_out& out, hipStream_t s) {
    const PolicyArgs Q{params, b.obs, nullptr, nullptr, n_params, p.layers, p.hidden, p.hidden_act, p.out_act};
    const PolicySpec& p2 = opp ? *opp : p;   // (without an opponent the second set is never read: opp_seats is 0)
    const PolicyArgs Q2{opp ? opp_params : params, b.obs, nullptr, nullptr, opp ? n_opp_params : n_params, p2.layers, p2.hidden, p2.hidden_act,
                        p2.out_act};
    const TeamArgs C{out.rewards, out.flags, (uint32_t)noise_seed, (uint32_t)(noise_seed >> 32)};
    const rsx_team_side_out &a = out.actor, &o = out.opponent;
    const SideArgs A{params, sigma, a.obs, a.actions, a.mean, a.sample, a.final_obs, a.next_obs, seats};
    const SideArgs O = opp ? SideArgs{opp_params, opp_sigma, o.obs, o.actions, o.mean, o.sample, o.final_obs, o.next_obs, opp_seats}
                           : SideArgs{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    const size_t lds = images_bytes(L, P.obs_dim, act_dim, P.n_blue, p, opp);
    if (phys) team_launch<true>(P, b, L, NR, phys, Q, Q2, C, A, O, lds, n_steps, s);
    else team_launch<false>(P, b, L, NR, nullptr, Q, Q2, C, A, O, lds, n_steps, s);
}

}  // namespace rsx
