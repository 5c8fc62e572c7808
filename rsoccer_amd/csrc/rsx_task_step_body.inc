// rsx_task_step_body.inc — the body of task_step_kernel and task_step_phys_kernel (rsx_kernels.hpp), included into both.
// Textual inclusion, not a shared device function: the literal kernels then compile to (nearly) the instructions they had
// before the per-env variant existed (an inlined body function moved registers and instructions around: -2 % on the VSS-v0
// headline).  Expects PHYS (constexpr bool) and `phys` (the physics block, or nullptr) in scope.  What a step shares with the lookahead
// (rsx_plan_body.inc) is text of its own, for the same reason: rsx_step_commands.inc, rsx_step_wire.inc, rsx_step_xr.inc.
// The paired form (rsx_pair.hpp: task_pair_step_kernel, RSX_STEP_PAIRED defined around the inclusion) runs this body with two waves
// per workgroup: the blocks under RSX_STEP_PAIRED split the work, and what the reward lane does is text of its own that the service
// wave includes instead (rsx_step_ball_load.inc, rsx_step_reward.inc, rsx_step_vss_metrics.inc, from rsx_step_service.inc).  Without
// the macro the preprocessed text is what it was before that form existed.
    // A multi-step launch is short of SGPRs, not of start-up latency: there the preloaded copies
    // are left dead and everything is fetched from the kernarg segment when it is needed.
    constexpr bool HOT = MODE != MODE_ROLLOUT;
    Params P = P_;
    Buffers bufs = bufs_;
    if (HOT) {
        RSX_UNPACK_HOT(P);
        bufs.state = hp_state; bufs.aux = hp_aux; bufs.actions = hp_in; bufs.flags = hp_flags;
    }
    const int n_steps_arg = hp_n_steps & RSX_N_STEPS_MASK;
    constexpr int mode = MODE == MODE_ROLLOUT ? MODE_STEP : MODE;
    const int n_steps = MODE == MODE_ROLLOUT ? n_steps_arg : 1;
    // the step counter of this launch (see step_tick): every workgroup — tiles, idle tail, placement helpers — takes part
    const bool tick_dev = __builtin_expect((hp_n_steps & RSX_TICK_DEV) != 0, 0);
    using K = KC<KIND>;
    using T = TC<TASK>;
    constexpr int G = 64 / L;
    constexpr int ID = T::info_dim;
    constexpr int AD = T::act_dim;
    __shared__ Shared<L> sh;
    // placement cache: single-step launches of the two rejection-sampled tasks in their fixed-size 8-lane variants
    // (VSS-v0 3v3 would qualify as well and was measured: five resets per 4096-env launch — its slowest wave is a contact wave,
    // 9.33 vs 9.30-9.38 us — for 112 B more reads per env-step; it keeps the inline placement)
    constexpr bool PC = !PHYS && MODE == MODE_STEP && L == 8 && TASK == RSX_TASK_SSL_STATIC_DEFENDERS && NR == 7;
    if constexpr (PC) {
        if (__builtin_expect(bufs.pcache != nullptr && (int)blockIdx.x >= hp_per_xcd * 8, 0)) {   // a helper workgroup (behind the tiles)
            const StepTick th = step_tick(tick_dev, P, bufs, 1u);
            if (th.ok) placement_helper<KIND, L, TASK, (PC ? NR : 1)>(P, bufs, (int)blockIdx.x - hp_per_xcd * 8, th.t, sh);
            return;
        }
    }
    StepTick tk{0u, true};
#ifdef RSX_STEP_PAIRED
    __shared__ PairBox pb;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // 0: the physics wave, 1: the service wave
    // the first 8 KB of code behind this point are touched by the service wave (CODE_PF below; taken here, where both waves pass, so
    // that the window starts at the head of the kernel whatever the layout of the two waves' code)
    unsigned long long code_pc;
    asm volatile("s_getpc_b64 %0" : "=s"(code_pc));
    if (tick_dev) {
        // a device-keyed handle: the physics wave reads, checks and advances the workgroup's slot, the service wave is handed the
        // result.  tick_dev is a launch argument: both waves are here or neither is
        if (wv == 0) {
            tk = step_tick(true, P, bufs, 1u);
            if (threadIdx.x == 0) { pb.tick = tk.t; pb.ok = tk.ok ? 1u : 0u; }
        }
        pair_barrier();
        if (wv != 0) tk = StepTick{(uint32_t)__builtin_amdgcn_readfirstlane((int)pb.tick), __builtin_amdgcn_readfirstlane((int)pb.ok) != 0};
    } else {
        tk = step_tick(false, P, bufs, 1u);
    }
    // the one early exit: the same value on both waves, taken by both, in front of barrier 1
    if (__builtin_expect(!tk.ok, 0)) return;
    const uint32_t tick0 = tk.t;
    const int lane = threadIdx.x & 63;
#else
    if (MODE == MODE_STEP || MODE == MODE_ROLLOUT) {
        tk = step_tick(tick_dev, P, bufs, (uint32_t)n_steps);
        if (__builtin_expect(!tk.ok, 0)) return;
    }
    const uint32_t tick0 = tk.t;
    const int lane = threadIdx.x;
#endif
    const int b = LaneMap<L>::body(lane), g = LaneMap<L>::env(lane);
    const int tile = tile_of_block(HOT ? hp_per_xcd : (int)(gridDim.x >> 3));
    const int e = tile * G + g;
    const int N = NR ? NR : P.n_robots;
    const bool live = e < P.num_envs;
    const bool is_robot = live && b < N, is_ball = live && b == N;
    const size_t B = (size_t)P.num_envs;
    const uint32_t env_id = P.env_id_base + (uint32_t)e;
    // observation width: a compile-time constant when the team sizes are (lets the copy-out unroll)
    constexpr int OD_C = obs_dim_c<TASK, NR>();
    const int OD = OD_C ? OD_C : P.obs_dim;
#define auxe(ROW) at_byte(bufs.aux, (ix_t)(ROW) * ((ix_t)4 * (ix_t)P.row_stride) + (ix_t)4 * (ix_t)e)   // row ROW of this env in the scalar arena
#ifdef RSX_STEP_PAIRED
    // (a workgroup of the idle tail behind the last tile has no live lane and still runs to the end on both waves: both barriers are met)
    // The included text is ONE braced block, the whole life of the service wave from here on, and its last statement is `return`:
    // nothing below this line runs on wave 1.  Keep it so — a service wave that fell through would run the physics wave's
    // barriers a second time and park its partner.
    if (wv != 0)
#include "rsx_step_service.inc"
#endif

#ifdef RSX_TIMING
    if (lane == 0) { sh.dbg = bufs.dbg; bufs.dbg[(size_t)13 * gridDim.x + blockIdx.x] = __builtin_amdgcn_s_memrealtime(); }  // 100 MHz, chip-wide
#endif
    RSX_STAMP(0);
    // ---- load ----
    Body o; float od, wd, wheels[4];
    const RawBody raw = load_raw<KIND>(P, bufs.state, e, b, is_robot, is_ball);
    // Every launch starts with a cold instruction cache (the first pass through the code costs ~1 k cycles more than the later ones,
    // profiles/r04_timeline_4096.txt).  The VSS single-step kernels touch the 8 KB of their own code that follow the entry point with
    // ONE data load — a lane per 128-byte line; it lands with the state loads, long before the wave gets there — so that those
    // instruction fetches find their lines in the L2: VSS-v0 at 4096 envs 9.02 -> 8.88 us per step (three interleaved rounds).
    // Measured per kernel: later windows (+4, +8, +12 KB) or 16 / 24 KB gain nothing; the SSL kernels lose (11v11 +4 %, 1v6 +0.5 %).
#ifdef RSX_STEP_PAIRED
    constexpr bool CODE_PF = false;   // (the service wave's load)
#else
    constexpr bool CODE_PF = !PHYS && KIND == RSX_KIND_VSS && MODE == MODE_STEP;   // (measured for the literal kernels only)
#endif
    uint32_t code_touch = 0;
    if (CODE_PF) {
        unsigned long long pc;
        asm volatile("s_getpc_b64 %0" : "=s"(pc));
        code_touch = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(pc) + 128u * (unsigned)lane));
    }
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
#ifndef RSX_STEP_PAIRED   // (the paired form: the service wave loads them)
#include "rsx_step_ball_load.inc"
#endif
    // metrics[0] (env-steps) is counted on the device by ONE lane of the grid: launches of a handle
    // are stream-ordered, so a plain read-modify-write is race free and costs no atomic
    const bool counts_steps = (MODE == MODE_STEP || MODE == MODE_ROLLOUT) && blockIdx.x == 0 && lane == 0;
    unsigned long long steps_before = 0;
    if (counts_steps) steps_before = bufs.metrics[0];
    float reward = 0.0f; int term = 0, trunc = 0;
    bool success = false;  // goal scored / course completed / pass received (metrics[2])
    bool against = false;  // goal conceded (metrics[3]; scrimmage)
    bool was_reset = false;
    // caller-fed actions of the agent lane (robot 0); fed launches run a single step
    const bool fed = MODE == MODE_STEP && bufs.actions != nullptr;
    float act[AD];
#pragma unroll
    for (int i = 0; i < AD; ++i) act[i] = 0.0f;
    if (TASK == RSX_TASK_SSL_SCRIMMAGE) {   // every robot is commanded: [B][N][4]
        if (fed && is_robot) {
#pragma unroll
            for (int i = 0; i < AD; ++i) act[i] = at_byte(bufs.actions, (ix_t)4 * (((ix_t)e * (ix_t)N + (ix_t)b) * (ix_t)AD + (ix_t)i));   // ([B][N][AD] is smaller than the state array)
        }
    } else if (fed && is_robot && b == 0) {
#pragma unroll
        for (int i = 0; i < AD; ++i) act[i] = at_byte(bufs.actions, (ix_t)4 * ((ix_t)e * (ix_t)AD + (ix_t)i));
    }

    // placement cache: this body's pose in the env's next episode and the episode id it was made for, loaded with the state
    float pcx = 0.0f, pcy = 0.0f, pcth = 0.0f;
    uint32_t ptag = 0u;
    bool pc_on = false;
    if constexpr (PC) {
        pc_on = bufs.pcache != nullptr;
        if (pc_on && (is_robot || is_ball)) {
            constexpr int NBD = (PC ? NR : 1) + 1;
            const float* const pr = bufs.pcache + (size_t)((tick0 + 1u) & 1u) * (size_t)pcache_rows<NBD>() * B;
            pcx = pr[(size_t)(0 * NBD + b) * B + e]; pcy = pr[(size_t)(1 * NBD + b) * B + e]; pcth = pr[(size_t)(2 * NBD + b) * B + e];
            ptag = __float_as_uint(pr[(size_t)(3 * NBD) * B + e]);
        }
    }

    // single-step launches: this step's random numbers, computed in the shadow of the loads
    StepDraw pre;
#ifndef RSX_STEP_PAIRED   // (the paired form: the service wave's, picked up behind the load wait)
    if (MODE == MODE_STEP) pre = draw_for_step<KIND, TASK>(P, env_id, tick0, b, is_robot, fed);
#endif

    // All loads land here, once.  Without this the compiler parks a vmcnt(0) at the top of the
    // step loop (loop-carried values come from loads on the first trip), and on gfx9-class
    // counters that wait also drains the previous trip's global STORES: one HBM write round
    // trip per env step in the multi-step (rollout) launches.
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    if (CODE_PF) asm volatile("" :: "v"(code_touch));   // (the value itself is of no interest)
#if defined(RSX_STEP_PAIRED) && RSX_PAIR_HEAD
    // The paired form's physics wave has no arithmetic in the shadow of its loads, so a second round trip is all exposed.  There was
    // one: the compiler placed the tail's `steps + 1` in the guarded block that loads the step counter, with a vmcnt(1) in front of it
    // that drains the state rows, and the OU rows, the env-step counter and the fed actions were issued behind it.  The loaded
    // scalars pass through here: no use of one can be scheduled ahead of the wait above.
    asm volatile("" : "+v"(steps), "+v"(episode), "+v"(ou0), "+v"(ou1));
#endif
    interpret_body<KIND>(raw, is_robot, is_ball, o, od, wd, wheels);
#ifdef RSX_STEP_PAIRED
    RSX_STAMP(22);
    // barrier 1 (both waves, unconditionally: no branch between the early exit above and this line): the service wave has published
    // this step's draws, and its loads of the step counter and the info rows have landed
    pair_barrier();
    {
        const float2 d2 = pb.dr[lane];
#pragma unroll
        for (int i = 0; i < 5; ++i) pre.v[i] = 0.0f;
        pre.v[0] = d2.x; pre.v[1] = d2.y;
    }
#endif
    RSX_STAMP(1);

    for (int it = 0; it < n_steps; ++it) {
        bool ended;
        const float obs_ts = prev_pot;   // the task scalar as this step's observation sees it (before the reward moves it)
        if (mode == 2) {
            const bool flagged = live && bufs.flags[2 * B + e] != 0;   // third row of the flags array: the env mask of rsx_task_reset_to
            if (flagged) {
                episode += 1; steps = 0; ou0 = 0.0f; ou1 = 0.0f;
                if constexpr (PHYS) phys_redraw(P, phys, e, env_id, episode, b == 0, cf);
                if (is_ball) {
#pragma unroll
                    for (int i = 0; i < 10; ++i) info[i] = 0.0f;
#pragma unroll
                    for (int i = 0; i < ID; ++i) auxe(ROW_INFO + i) = 0.0f;
                    ep_ret = 0.0f; prev_pot = 0.0f;
                }
            }
            // (only the re-placed envs: the observation of an env the mask leaves alone stays the one its last step wrote — recomputed here
            // it would see the task scalar AFTER that step's reward moved it, e.g. the checkpoint count of SSLDribbling; found by
            // tests/test_gpu_api_fuzz.py in 3 of 500 sequences)
            if (flagged) write_obs<KIND, TASK>(P, bufs.obs + (size_t)e * OD, b, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd, o.ir, prev_pot);
            wave_sync();
            ended = false;
        } else if (mode == 1) {
            // reset(): nothing to simulate; fall through to the placement block below
            ended = live;
            episode += 1;
            if (is_ball) {
#pragma unroll
                for (int i = 0; i < 10; ++i) info[i] = 0.0f;
#pragma unroll
                for (int i = 0; i < ID; ++i) auxe(ROW_INFO + i) = 0.0f;   // like reset_to above: the info rows of a fresh episode read zero
                ep_ret = 0.0f; prev_pot = 0.0f;
            }
        } else {
            const bool first_step = steps == 0;
            const uint32_t t = tick0 + (uint32_t)it;   // per-step draws are keyed by the handle's step count, not by the env's counters
            if (is_ball && first_step) {
#pragma unroll
                for (int i = 0; i < 10; ++i) info[i] = 0.0f;
                ep_ret = 0.0f;
            }
            const float lastx = o.x, lasty = o.y;  // the reference's last_frame (pre-step)

            // ---- actions -> commands ----
            float q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const StepDraw dr = MODE == MODE_STEP ? pre : draw_for_step<KIND, TASK>(P, env_id, t, b, is_robot, fed);
#include "rsx_step_commands.inc"

            // ---- physics ----
            RSX_STAMP(2);
            // the sub-step cuts (rsx_contact.hpp: SubstepCuts) of the VSS-v0 3v3 eight-lane single-step kernels with literal coefficients,
            // per kernel as measured; every other instantiation: none
#ifdef RSX_STEP_PAIRED
            constexpr int CUTS = RSX_SUBSTEP_CUTS_PAIR;
#else
            constexpr int CUTS = !PHYS && KIND == RSX_KIND_VSS && TASK == RSX_TASK_VSS_V0 && L == 8 && NR == 6 && MODE == MODE_STEP ? RSX_SUBSTEP_CUTS_LANES : 0;
#endif
            physics<KIND, L, NR, SubstepCuts<(CUTS & 1) != 0, (CUTS & 2) != 0, (CUTS & 4) != 0, (CUTS & 8) != 0, (CUTS & 16) != 0>>(P, o, b, g, live, sh, cf);
            RSX_STAMP(3);
            if (MODE == MODE_STEP && KIND == RSX_KIND_SSL) {
                // Single-step launches of the SSL tasks: what the rest of the step reads of the parameter block is fetched from the kernarg
                // segment HERE, behind an opaque pointer, instead of being loaded at the kernel's entry and parked in VGPR lanes across
                // the physics (these kernels run out of scalar registers: ~40 v_writelane at entry, ~60 v_readlane after the physics)
                typedef const __attribute__((address_space(4))) uint32_t* kw_t;
                constexpr size_t KOFF = RSX_PARAMS_KERNARG_OFFSET;   // after RSX_HOT_ARGS
                static_assert(sizeof(Params) % 4 == 0 && KOFF % 4 == 0, "parameter block in dwords");
                kw_t pk = (kw_t)__builtin_amdgcn_kernarg_segment_ptr() + KOFF / 4;
                asm volatile("" : "+s"(pk));
                struct Words { uint32_t w[sizeof(Params) / 4]; } raw;
#pragma unroll
                for (size_t i = 0; i < sizeof(Params) / 4; ++i) raw.w[i] = pk[i];
                P = __builtin_bit_cast(Params, raw);
                RSX_UNPACK_HOT(P);
            }

            // ---- wire-format values, observation, reward ----
#ifdef RSX_STEP_PAIRED
#include "rsx_step_pair_tail.inc"   // (hand-over to the service wave right behind physics(), then the wire format and the observation)
#else
#include "rsx_step_wire.inc"
            write_obs<KIND, TASK>(P, bufs.obs + (size_t)e * OD, b, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd, o.ir, obs_ts);
#include "rsx_step_xr.inc"   // what the reward lane (the ball's) needs from the robots' lanes -> sh.x0[g]
            wave_sync();
#include "rsx_step_reward.inc"
#endif
        }

        RSX_STAMP(4);
        // ---- episode end: same-step auto-reset (or reset()) ----
        if (RSX_RARE_B(KIND, 4, __any(ended))) {
            if (ended && mode == 0) {  // terminal observation
                write_obs<KIND, TASK>(P, bufs.final_obs + (size_t)e * OD, b, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd, o.ir, obs_ts);
            }
            if (ended && mode == 0) episode += 1;   // every lane of the env: the new episode's id
            if (KIND == RSX_KIND_VSS) {
#ifndef RSX_STEP_PAIRED   // (the paired form: the service wave holds the info terms and adds the counters)
#include "rsx_step_vss_metrics.inc"
#endif
            } else if (mode == 0) {
                // SSL tasks (short episodes: several resetting waves in every launch): the ball lane
                // holds the increments, lanes 0..5 of the env add one each, so the wave issues ONE
                // atomic instruction instead of six guarded ones, each wrapped in wave-reduction
                // code by the compiler.  Measured: static defenders 11.33 -> 11.03 us; VSS-v0 does
                // not gain (8.83 -> 8.88) and keeps the plain form.
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
            RSX_STAMP(15);
            // an env whose next episode's poses were in the cache takes them from there; the others are placed here
            const bool hit = PC && pc_on && ended && ptag == episode;
            const bool place = ended && !hit;
            const bool any_place = !PC || __any(place);
            if (any_place) {
                if (place) place_predraw<TASK, L>(P, env_id, episode, b, sh.draws[g]);
                wave_sync();  // draws published; stage rows of ended envs are about to be overwritten
            }
            RSX_STAMP(16);
            float4 pz = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            // A single-step launch waits for its slowest wave, which is one that resets an env:
            // there the placement runs in its parallel form.  A multi-step launch pays for the
            // average wave instead, and the sequential form issues fewer instructions.
            if (TASK == RSX_TASK_SSL_SCRIMMAGE) {
                // robot k in cell (k % 6, k / 6) of a 6 x 4 grid, one Philox block per body: every lane places itself
                if (ended && (is_robot || is_ball)) {
                    const u32x4 u = philox4x32(env_id, episode, (uint32_t)b, DOM_PLACE, P.key0, P.key1);
                    const float jx = u01(u.x) * 2.0f - 1.0f, jy = u01(u.y) * 2.0f - 1.0f;
                    if (is_ball) pz = make_float4(P.sc_jb * jx, P.sc_jb * jy, 0.0f, 0.0f);
                    else pz = make_float4(P.sc_sx * ((float)(b % 6) - 2.5f) + P.sc_j * jx,
                                          P.sc_sy * ((float)(b / 6) - 1.5f) + P.sc_j * jy, 360.0f * u01(u.z), 0.0f);
                }
            } else if ((TASK == RSX_TASK_VSS_V0 || TASK == RSX_TASK_SSL_STATIC_DEFENDERS) && MODE != MODE_ROLLOUT) {
                if (any_place && place) pz = place_env_parallel<TASK, L, NR>(P, N, env_id, episode, b, g, is_robot, sh.A, sh.draws[g]);
                if (hit) pz = make_float4(pcx, pcy, pcth, 0.0f);
                if (PC && pc_on && bufs.pcstats && ended && is_ball) atomicAdd(&bufs.pcstats[hit ? 0 : 1], 1ull);
            } else {
                if (ended && is_ball) place_env<TASK, L>(P, N, env_id, episode, g, sh.A, sh.draws[g]);
                wave_sync();
                if (ended && (is_robot || is_ball)) pz = sh.A[LaneMap<L>::slot(b, g)];
            }
            RSX_STAMP(17);
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
                write_obs<KIND, TASK>(P, bufs.obs + (size_t)e * OD, b, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd, 0, 0.0f);
            }
            wave_sync();
            RSX_STAMP(18);
        }

        wave_sync();
    }

    RSX_STAMP(5);
    // ---- store (wire format: degrees, deg/s; SSL: infrared + wheel speeds) ----
    if (mode != 2) store_body<KIND>(P, bufs.state, e, b, is_robot, is_ball, o, od, wd, wheels, P.n_sub != 0 || was_reset);
    if (live && b == 0) {
        auxe(ROW_STEPS) = __int_as_float(steps);
        auxe(ROW_EPISODE) = __uint_as_float(episode);
    }
    if (TASK == RSX_TASK_VSS_V0 && is_robot && b >= 1) {
        auxe(ROW_OU + 2 * b) = ou0; auxe(ROW_OU + 2 * b + 1) = ou1;
    }
#ifndef RSX_STEP_PAIRED   // (the paired form: the service wave's store)
    if (is_ball) {
        auxe(ROW_PREV_POT) = prev_pot;
        if (TASK != RSX_TASK_VSS_V0) auxe(ROW_EP_RET) = ep_ret;
    }
#endif
#undef auxe
    if (counts_steps) bufs.metrics[0] = steps_before + (unsigned long long)P.num_envs * (unsigned long long)n_steps;
    RSX_STAMP(6);
#ifdef RSX_TIMING
    __builtin_amdgcn_s_waitcnt(0x0F70);
    RSX_STAMP(7);
    if (lane == 0) bufs.dbg[(size_t)14 * gridDim.x + blockIdx.x] = __builtin_amdgcn_s_memrealtime();
#endif
