// rsx_contact.hpp — the contact physics of the lane-group kernels: the n_sub sub-steps of one env.step() for the body a lane
// holds (physics; one sub-step is the text of rsx_substep_body.inc), its contact sweeps (the unrolled VSS walk inside the sub-step,
// vss_sweep_loop, ssl_sweep) over the LDS snapshot, what the VSS-v0 3v3 single-step kernels cut from a sub-step's control flow
// (SubstepCuts), and the per-env coefficients of a physics-enabled handle (load_coefs, phys_redraw).  The per-body arithmetic is
// rsx_body.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "rsx_math.hpp"
#include "rsx_params.hpp"
#include "rsx_body.hpp"
#include "rsx_phys.hpp"
#include "rsx_lane_map.hpp"

namespace rsx {

// ---- per-env physics (rsx_phys.hpp) ----
// the env's coefficients into registers: one load per row, once per launch
__device__ __forceinline__ void load_coefs(const Params& P, const float* __restrict__ phys, const int e, EnvCoef& cf) {
    const float* const rows = phys + PHYS_HDR_FLOATS + (size_t)NPHYS * (size_t)P.row_stride;
    const ix_t B4 = (ix_t)4 * (ix_t)P.row_stride, off = (ix_t)4 * (ix_t)e;
#pragma unroll
    for (int i = 0; i < NCOEF; ++i) cf.c[i] = at_byte(rows, off + (ix_t)i * B4);
}
// Episode start of env e (every lane of the env calls this): the parameters with a randomisation range are redrawn —
// lo + (hi - lo) * u01(x), x from philox4x32(env_id, episode, p, DOM_PHYS) — and the coefficients re-derived; `writer` (one lane
// of the env) stores both.  Nothing happens while no range is set.
__device__ __forceinline__ void phys_redraw(const Params& P, float* __restrict__ phys, const int e, const uint32_t env_id,
                                            const uint32_t episode, const bool writer, EnvCoef& cf) {
    const PhysHeader* const hd = reinterpret_cast<const PhysHeader*>(phys);
    const uint32_t mask = hd->mask;
    if (mask == 0u) return;
    const size_t S = (size_t)P.row_stride;
    float* const raw = phys_raw(phys);
    float v[NPHYS];
#pragma unroll
    for (int p = 0; p < NPHYS; ++p) {
        if ((mask >> p) & 1u) {
            const u32x4 u = philox4x32(env_id, episode, (uint32_t)p, DOM_PHYS, P.key0, P.key1);
            v[p] = hd->lo[p] + (hd->hi[p] - hd->lo[p]) * u01(u.x);
        } else {
            v[p] = raw[(size_t)p * S + e];
        }
    }
    derive_coefs(hd->kind, hd->ts_ms, v, cf.c);
    if (writer) {
        float* const co = phys_coef(phys, S);
#pragma unroll
        for (int p = 0; p < NPHYS; ++p)
            if ((mask >> p) & 1u) raw[(size_t)p * S + e] = v[p];
#pragma unroll
        for (int i = 0; i < NCOEF; ++i) co[(size_t)i * S + e] = cf.c[i];
    }
}

// VSS contact sweep with a run-time partner loop: exact integer overlap test into one bit per
// partner, then the lane walks ITS partners in index order.  First sweep of the run-time-count
// kernels and second sweep (rare) of all VSS kernels.  Returns whether some pair was deep.
template <int KIND, int L, class CF = LitCoef<KIND>>
__device__ __forceinline__ bool vss_sweep_loop(const Params& P, Body& o, const int N, const int g, const bool is_ball,
                                               const bool ball_low, const Shared<L>& sh, bool& wallp, const float2 fo, const CF& cf = CF{}) {
    using K = KC<KIND>;
    constexpr int G = 64 / L;
    constexpr uint32_t T_RR = __builtin_bit_cast(uint32_t, K::rs_rr2) - 1u;
    constexpr uint32_t T_RB = __builtin_bit_cast(uint32_t, K::rs_rb2) - 1u;
    unsigned todo = 0;
#pragma unroll 4
    for (int j = 0; j <= N; ++j) {
        const float4 oj = sh.A[LaneMap<L>::slot(j, g)];
        const bool rb = is_ball || j == N;
        const float dx = oj.x - o.x, dy = oj.y - o.y;
        const uint32_t u = __float_as_uint(fma_(dx, dx, dy * dy)) - 1u;   // own slot: 0xFFFFFFFF
        todo |= ((u < (rb ? T_RB : T_RR)) & (!rb | ball_low)) ? 1u << j : 0u;
    }
    if (todo == 0) return false;
    const bool v2w = K::wall_aware && __ballot(!is_ball && at_wall<KIND>(P, o.x, o.y)) != 0ull;   // (rsx_body.hpp: contact_response)
    bool deep = false;
    float avx = 0.0f, avy = 0.0f, apx = 0.0f, apy = 0.0f, aw = 0.0f;
    const Body snap = o;   // every partner is evaluated against the snapshot
    const float lever = is_ball ? K::r_ball : K::r_robot;
    while (todo) {
        const int j = __builtin_ctz(todo);
        todo &= todo - 1;
        const float4 oj = sh.A[LaneMap<L>::slot(j, g)];
        const float wj = sh.W[LaneMap<L>::slot(j, g)];
        const float2 fj = sh.F[LaneMap<L>::slot(j, g)];
        const float dx = oj.x - o.x, dy = oj.y - o.y;
        const bool rb = is_ball || j == N;
        contact_response<KIND>(P, snap, oj, fma_(dx, dx, dy * dy), rb ? K::rs_rb : K::rs_rr, rb ? cf.ope_rb() : cf.ope_rr(),
                         is_ball ? cf.w_rb_b() : (j == N ? cf.w_rb_r() : K::w_rr),
                         is_ball ? cf.kt_rb_b() : (j == N ? cf.kt_rb_r() : K::kt_rr), rb ? cf.mu_rb() : cf.mu_rr(),
                         is_ball ? K::spin_c : 0.0f, fma_(wj, j == N ? K::r_ball : K::r_robot, snap.om * lever),
                         K::beta, K::pen2, !rb, v2w, avx, avy, apx, apy, aw, deep, wallp, fo, fj);
    }
    // only a body that touched something is updated (the others keep their bits)
    o.vx = o.vx + avx; o.vy = o.vy + avy;
    o.x = o.x + apx; o.y = o.y + apy;
    if (is_ball) o.om = o.om + aw;
    return deep;
}

// What the kicker / dribbler of some robot decided for the ball in the first sweep of a sub-step
// u[j] = bits(|p_j - p_o|^2) - 1 for the SLOTS bodies of the lane's env, two partners per packed-FP32 instruction
// (v_pk_add / v_pk_mul / v_pk_fma are IEEE per component: the same bits as the scalar form), positions from the
// [env][body] copies in LDS (one 16-byte read = four partners).
struct NoFill { __device__ __forceinline__ void operator()() const {} };
// `fill`: work that does not depend on the partners' positions, issued between the LDS reads and their first use (the reads take
// ~100 cycles to come back and a lone wave has nothing else to run meanwhile)
template <int SLOTS, int L, typename FILL = NoFill>
__device__ __forceinline__ void overlap_keys_packed(const Shared<L>& sh, const int g, const float ox, const float oy, uint32_t* u, FILL fill = FILL{}) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    typedef float f4 __attribute__((ext_vector_type(4)));
    constexpr int Q = (SLOTS + 3) / 4;
    const f4* X4 = reinterpret_cast<const f4*>(&sh.X[g * L]);
    const f4* Y4 = reinterpret_cast<const f4*>(&sh.Y[g * L]);
    f4 xs[Q], ys[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) { xs[q] = X4[q]; ys[q] = Y4[q]; }
    fill();   // (in program order behind the reads; a sched_barrier here keeps the compiler from peeling the sweep loop and costs scratch)
    const f2 ox2 = {ox, ox}, oy2 = {oy, oy};
#pragma unroll
    for (int q = 0; q < Q; ++q) {
#pragma unroll
        for (int hlf = 0; hlf < 2; ++hlf) {
            const int j = 4 * q + 2 * hlf;
            if (j >= SLOTS) continue;
            const f2 px = hlf ? xs[q].zw : xs[q].xy, py = hlf ? ys[q].zw : ys[q].xy;
            const f2 dx = px - ox2, dy = py - oy2;
            const f2 t = dy * dy;
            const f2 d2 = __builtin_elementwise_fma(dx, dx, t);
            u[j] = __float_as_uint(d2.x) - 1u;
            if (j + 1 < SLOTS) u[j + 1] = __float_as_uint(d2.y) - 1u;
        }
    }
}

struct BallOverride { bool ovr, okick; float ovx, ovy, ovz; };

// SSL contact sweep.  Robot lanes: robot-robot pairs (circles), then the robot's own robot-ball
// geometry (kicker mouth or body circle) whose ball-side record goes to LDS; one ballot tells the
// ball lane which robots wrote one.  FIRST: infrared is refreshed and kicker / dribbler act.
// NRX > 0: robot count known at compile time.  `first` is wave-uniform: both sweeps of a sub-step run
// the SAME instructions (a second copy of this code would be cold in the instruction cache every
// time it is needed, which costs more than the sweep itself).
template <int KIND, int L, int NRX, class CF = LitCoef<KIND>>
__device__ __forceinline__ bool ssl_sweep(const Params& P, Body& o, const int N, const int g, const int lane,
                                          const bool is_robot, const bool is_ball, const bool ball_low,
                                          const bool first, Shared<L>& sh, BallOverride& bo, bool& wallp, const CF& cf = CF{}) {
    using K = KC<KIND>;
    constexpr int G = 64 / L;
    constexpr uint32_t T_RR = __builtin_bit_cast(uint32_t, K::rs_rr2) - 1u;
    int fl = 0;   // what this robot does to the ball in this sweep (0 = nothing)
    bool touched = false;   // deep contact seen by this lane
    bool got = false;       // this body touched something: only then is it updated
    float avx = 0.0f, avy = 0.0f, apx = 0.0f, apy = 0.0f, aw = 0.0f;
    if (is_robot) {
        unsigned todo = 0;
        if (NRX) {
            uint32_t u[NRX ? NRX : 1];   // exact integer form of 0 < d2 < rs_rr^2, see the VSS sweep
            overlap_keys_packed<(NRX ? NRX : 1), L>(sh, g, o.x, o.y, u);
            uint32_t um = u[0];
#pragma unroll
            for (int j = 1; j < NRX; ++j) um = min(um, u[j]);
            if (RSX_RARE_B(KIND, 2, um < T_RR)) {
#pragma unroll
                for (int j = NRX - 1; j >= 0; --j)   // slot j ends at bit j: shifted in from the right, highest slot first (a compare and an add-with-carry per slot, no bit constant in a register)
                    asm("v_cmp_gt_u32_e32 vcc, %2, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc" : "+v"(todo) : "v"(u[j]), "s"(T_RR) : "vcc");
            }
        } else {
#pragma unroll 4
            for (int j = 0; j < N; ++j) {
                const float4 oj = sh.A[LaneMap<L>::slot(j, g)];
                const float dx = oj.x - o.x, dy = oj.y - o.y;
                todo |= (__float_as_uint(fma_(dx, dx, dy * dy)) - 1u) < T_RR ? 1u << j : 0u;
            }
        }
        if (RSX_RARE_B(KIND, 2, todo != 0)) {   // per-lane partner walk, see the VSS sweep
            bool& deep = touched;
            got = true;
            const bool v2w = K::wall_aware && __ballot(at_wall<KIND>(P, o.x, o.y)) != 0ull;   // some robot of the wave (that has a partner) at a wall
            // Two copies of the walk, picked by that wave-uniform flag: the usual one holds v1's instructions and nothing else, the wall-
            // aware one (model v2) sits behind it — a test per partner inside ONE loop put the wall code's branches into the hot loop body
            auto walk = [&](auto wall_tag) {
                constexpr bool WALLS = decltype(wall_tag)::value;
                // software-pipelined like the VSS walk: the next partner's slot is fetched while the current response is computed
                int jn = __builtin_ctz(todo);
                todo &= todo - 1;
                float4 nxt = sh.A[LaneMap<L>::slot(jn, g)];
                float nxw = sh.W[LaneMap<L>::slot(jn, g)];
                for (;;) {
                    const float4 oj = nxt;
                    const float wj = nxw;
                    const bool more = todo != 0;
                    if (more) {
                        jn = __builtin_ctz(todo);
                        todo &= todo - 1;
                        nxt = sh.A[LaneMap<L>::slot(jn, g)];
                        nxw = sh.W[LaneMap<L>::slot(jn, g)];
                    }
                    const float dx = oj.x - o.x, dy = oj.y - o.y;
                    contact_response<KIND>(P, o, oj, fma_(dx, dx, dy * dy), K::rs_rr, cf.ope_rr(), K::w_rr, K::kt_rr, cf.mu_rr(), 0.0f,
                                           fma_(wj, K::r_robot, o.om * K::r_robot), K::beta, K::pen2, true, L == 8 ? WALLS : v2w, avx, avy, apx, apy, aw, deep, wallp);
                    if (!more) break;
                }
            };
            // (measured, us per step v1 / one loop / two copies: 1v6 at 2048 envs, 8 lanes: 9.28 / 9.82 / 9.48; 11v11 at 1024 envs, 32 lanes:
            // 9.71 / 10.00 / 10.10 — each width keeps its better form)
            if constexpr (L == 8) { if (__builtin_expect(v2w, 0)) walk(std::true_type{}); else walk(std::false_type{}); }
            else walk(std::true_type{});
        }
        // robot - ball: kicker mouth (flat face at dck) or body circle; n points robot -> ball
        const float4 ob = sh.A[LaneMap<L>::slot(N, g)];
        float dx = ob.x - o.x, dy = ob.y - o.y;
        float nx = 0.0f, ny = 0.0f, pen = -1.0f;
        bool mouth = false, touch = false;
        // a mouth, circle or infrared contact needs the ball's centre within 0.126 m of the robot's ((dck_rb + ir_tol)^2
        // + half_kw^2 = 0.126^2, and rs_rb < 0.126): everything farther away skips the geometry (same values when taken)
        constexpr float NEAR2 = 0.13f * 0.13f;
        const float d2 = fma_(dx, dx, dy * dy);
        if (ball_low && d2 < NEAR2) {
            float lx = fma_(dx, o.c, dy * o.s), ly = fma_(dy, o.c, -(dx * o.s));
            if (fabsf(ly) < K::half_kw && lx > 0.0f) {
                mouth = true; pen = K::dck_rb - lx; nx = o.c; ny = o.s; touch = pen > 0.0f;
            } else {
                if (d2 < K::rs_rb2 && d2 > 0.0f) {
                    float d = sqrtf(d2), inv = 1.0f / d;
                    nx = dx * inv; ny = dy * inv; pen = K::rs_rb - d; touch = true;
                }
            }
        }
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float dws = 0.0f;
        if (touch) {
            touched |= pen > K::pen2;
            got = true;
            const float dvx = ob.z - o.vx, dvy = ob.w - o.vy;
            float vn = fma_(dvx, nx, dvy * ny);
            if (vn < 0.0f) {
                const float omb = sh.W[LaneMap<L>::slot(N, g)];
                float q = cf.ope_rb() * vn * cf.w_rb_r(); avx = fma_(q, nx, avx); avy = fma_(q, ny, avy);
                const float wsum = fma_(omb, K::r_ball, o.om * (mouth ? K::dck : K::r_robot));
                const float vt = fma_(dvy, nx, -(dvx * ny)) - wsum;
                const float lim = q * cf.mu_rb();
                const float ft = clampf(vt * cf.kt_rb_r(), lim, -lim);
                avx = fma_(-ft, ny, avx); avy = fma_(ft, nx, avy);
                // the ball's side of the same contact
                float qb = cf.ope_rb() * vn * cf.w_rb_b();
                const float limb = qb * cf.mu_rb();
                const float ftb = clampf(vt * cf.kt_rb_b(), limb, -limb);
                r0.x = fma_(-ftb, ny, qb * nx); r0.y = fma_(ftb, nx, qb * ny); dws = ftb * K::spin_c; fl |= 1;
            }
            float pc = K::beta * pen * cf.w_rb_r();
            apx = fma_(-pc, nx, apx); apy = fma_(-pc, ny, apy);
            float pb = K::beta * pen * cf.w_rb_b(); r0.z = pb * nx; r0.w = pb * ny; fl |= 2;
        }
        if (first) {
            o.ir = mouth && pen > -K::ir_tol;
            if (o.ir) {  // infrared: kicker / dribbler act on the ball
                if (o.kick_x > 0.0f || o.kick_z > 0.0f) {
                    fl |= 4 | 8;
                    r1.y = o.vx + o.kick_x * o.c; r1.z = o.vy + o.kick_x * o.s; r1.w = o.kick_z;
                } else if (o.drib) {
                    float hx = o.x + K::dck_rb * o.c, hy = o.y + K::dck_rb * o.s;
                    float cvx = (hx - ob.x) * P.drib_gain, cvy = (hy - ob.y) * P.drib_gain;
                    float m2 = cvx * cvx + cvy * cvy;
                    if (m2 > K::drib_vmax2) { float sc = K::drib_vmax / sqrtf(m2); cvx = cvx * sc; cvy = cvy * sc; }
                    fl |= 4;
                    r1.y = (o.vx - o.om * K::dck_rb * o.s) + cvx;
                    r1.z = (o.vy + o.om * K::dck_rb * o.c) + cvy;
                }
            }
        }
        r1.x = __int_as_float(fl);
        if (fl) { sh.Bq[lane] = r0; sh.Cq[lane] = r1; sh.Dq[lane] = dws; }
    }
    // which robots wrote a record: one ballot; the ball lane visits only those, in index order
    // (usually none: no LDS read at all on the ball's side)
    const unsigned long long wrote = __ballot(fl != 0);
    wave_sync();
    if (is_ball) {
        unsigned long long todo = L <= 32 ? (env_lane_mask<L>(g) & wrote) : wrote;
        while (todo) {
            const int lj = __builtin_ctzll(todo);
            todo &= todo - 1;
            const float4 r1 = sh.Cq[lj];
            const float4 r0 = sh.Bq[lj];
            const int flj = __float_as_int(r1.x);
            if (flj & 1) { avx = avx - r0.x; avy = avy - r0.y; aw = aw + sh.Dq[lj]; }
            if (flj & 2) { apx = apx + r0.z; apy = apy + r0.w; got = true; }
            if (flj & 4) { bo.ovr = true; bo.okick = (flj & 8) != 0; bo.ovx = r1.y; bo.ovy = r1.z; bo.ovz = r1.w; }
        }
    }
    if (got) {   // only a body that touched something is updated (the others keep their bits)
        o.vx = o.vx + avx; o.vy = o.vy + avy;
        o.x = o.x + apx; o.y = o.y + apy;
        if (is_ball) o.om = o.om + aw;
    }
    return touched;
}

// What physics() may cut from the control flow of a VSS sub-step with a compile-time robot count.  Every compare -> scalar ->
// s_and_saveexec -> s_cbranch_execz chain is a stall that a lone wave cannot overlap with anything, and a single-step launch lasts
// as long as its slowest wave, which is one that walks partners in every sub-step.  Each cut leaves the arithmetic as it is (same
// operations, same operands, same bits); which kernel takes which is measured per kernel (profiles/LABBOOK.md) and chosen by the
// caller (rsx_task_step_body.inc).  NoSubstepCuts is every other kernel's: the instructions they had before the switches existed.
//   GROUNDED   one ballot per step() of "is some ball of the wave in flight"; if none is, the sub-steps run without the flight gate
//              and without the ball-height ballot (ball_low is the constant true).  In VSS nothing launches the ball (no kicker) and
//              ball_flight, the only writer of z / vz, is entered only when one of them is positive: a ball that is down at the start
//              of a step stays down.  An airborne ball is caller-set state, and its wave runs the general loop, laid out behind.
//   VN_SELECT  respond_axes computes the normal impulse for every walking lane and keeps the old sums by select (rsx_body.hpp)
//   PREFETCH   the walk fetches the next partner's slot in every iteration; with no partner left, the current one's again
//   EXCHANGE_ALL  every lane publishes its snapshot (and its held axes) and computes the overlap keys in every sweep, without the
//              `active` guards; `any` is masked with `active` instead (which starts as the lane's role, robot or ball, and only
//              shrinks).  A lane writes its own LDS slots and reads its own env's, and slot L - 1 of an env, the idle lane's, is read
//              by nobody: what an idle or inactive lane publishes and tests disturbs no other lane
//   ACT_SELECT the actuation and the heading advance run on every lane; the lanes that are no robot keep their bits by select
// (A fourth, leaving a sweep in which no lane of the wave has a touching pair ahead of the deep ballot, was measured and lost on both
// kernels, alone and on top of these three: profiles/LABBOOK.md.)
template <bool GROUNDED, bool VN_SELECT, bool PREFETCH, bool EXCHANGE_ALL = false, bool ACT_SELECT = false>
struct SubstepCuts {
    static constexpr bool grounded = GROUNDED, vn_select = VN_SELECT, prefetch = PREFETCH, exchange_all = EXCHANGE_ALL, act_select = ACT_SELECT;
};
using NoSubstepCuts = SubstepCuts<false, false, false>;
// The cuts of the two kernels that take any, as bits (1 GROUNDED, 2 VN_SELECT, 4 PREFETCH, 8 EXCHANGE_ALL, 16 ACT_SELECT):
// task_pair_step_kernel<0,8,1,6,0> and task_step_kernel<0,8,1,6,0>, each with what it measured best with (profiles/LABBOOK.md): the
// paired kernel all five; the one-wave kernel the first three (the last two gain 2.2-2.6 % there, under three times its run-to-run range).
// A -D on the compiler's line builds another combination (tools/build_variant.py) for an A/B.
#ifndef RSX_SUBSTEP_CUTS_PAIR
#define RSX_SUBSTEP_CUTS_PAIR 31
#endif
#ifndef RSX_SUBSTEP_CUTS_LANES
#define RSX_SUBSTEP_CUTS_LANES 7
#endif

// ---------------------------------------------------------------------------------------------
// n_sub sub-steps of one env.step() for the body held by this lane.
//   b = body index of the lane (0..N-1 robots, N ball, > N idle), g = env slot in the wave
//   NR > 0: robot count known at compile time (pair loops fully unrolled); NR == 0: run-time
//   SC: SubstepCuts (VSS with NR > 0 only)
// ---------------------------------------------------------------------------------------------
template <int KIND, int L, int NR, class SC = NoSubstepCuts, class CF = LitCoef<KIND>>
__device__ __forceinline__ void physics(const Params& P, Body& o, const int b, const int g,
                                        const bool live, Shared<L>& sh, const CF& cf = CF{}) {
    static_assert(std::is_same<SC, NoSubstepCuts>::value || (KIND == RSX_KIND_VSS && NR > 0), "the sub-step cuts exist for the unrolled VSS walk");
    using K = KC<KIND>;
    constexpr int G = 64 / L;
    const int N = NR ? NR : P.n_robots;
    const bool is_robot = live && b < N;
    const bool is_ball = live && b == N;
    const int lane = LaneMap<L>::slot(b, g);

    // rolling resistance: a constant deceleration, applied once for the whole step() while the
    // ball is on the ground (exact stop, never reverses) — keeps the sqrt + divide chain out of
    // the sub-step loop, where the ball lane's branch is serialised with the robots' work.
    // Same place: the spin about the vertical axis decays at a constant rate to an exact stop.
    if (is_ball) ball_step_friction(P, o, cf);
#ifdef RSX_TIMING_SUB   // development: where a sub-step's cycles go (sub-steps 1.. only; tools/exp_substep_phases.py)
    unsigned long long tsA = 0, tsB = 0, tsC = 0, ts0 = 0, ts1 = 0, ts2 = 0;
#endif

    if constexpr (SC::grounded) {
        // one chain per step(): is some ball of the wave in flight (or holds a NaN: the general loop's own compares decide then)?
        const bool flying = __ballot(is_ball && !(o.z <= 0.0f && o.vz <= 0.0f)) != 0ull;
        if (__builtin_expect(!flying, 1)) {
            for (int sub = 0; sub < P.n_sub; ++sub) {
                constexpr bool ON_GROUND = true;
#include "rsx_substep_body.inc"
            }
        } else {   // caller-set state (rsx_set_state, a checkpoint, a write into the state tensor): the loop every other kernel runs
            for (int sub = 0; sub < P.n_sub; ++sub) {
                constexpr bool ON_GROUND = false;
#include "rsx_substep_body.inc"
            }
        }
    } else {
        for (int sub = 0; sub < P.n_sub; ++sub) {
            constexpr bool ON_GROUND = false;
#include "rsx_substep_body.inc"
        }
    }
#ifdef RSX_TIMING_SUB
    if (threadIdx.x == 0 && sh.dbg) {
        sh.dbg[(size_t)15 * gridDim.x + blockIdx.x] = tsA; sh.dbg[(size_t)16 * gridDim.x + blockIdx.x] = tsB; sh.dbg[(size_t)17 * gridDim.x + blockIdx.x] = tsC;
    }
#endif
}

}  // namespace rsx
