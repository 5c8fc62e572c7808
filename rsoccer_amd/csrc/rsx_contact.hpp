// rsx_contact.hpp — the contact physics of the lane-group kernels: the n_sub sub-steps of one env.step() for the body a lane
// holds (physics), its contact sweeps (the unrolled VSS walk inside physics, vss_sweep_loop, ssl_sweep) over the LDS snapshot,
// and the per-env coefficients of a physics-enabled handle (load_coefs, phys_redraw).  The per-body arithmetic is rsx_body.hpp's.
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

// ---------------------------------------------------------------------------------------------
// n_sub sub-steps of one env.step() for the body held by this lane.
//   b = body index of the lane (0..N-1 robots, N ball, > N idle), g = env slot in the wave
//   NR > 0: robot count known at compile time (pair loops fully unrolled); NR == 0: run-time
// ---------------------------------------------------------------------------------------------
template <int KIND, int L, int NR, class CF = LitCoef<KIND>>
__device__ __forceinline__ void physics(const Params& P, Body& o, const int b, const int g,
                                        const bool live, Shared<L>& sh, const CF& cf = CF{}) {
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

    for (int sub = 0; sub < P.n_sub; ++sub) {
#ifdef RSX_TIMING_SUB
        ts0 = __builtin_readcyclecounter();
#endif
        // ---- A: actuation + integration ----
        if (is_robot) {   // rsx_body.hpp: the per-body arithmetic is stated once for all kernel layouts
            actuate_robot<KIND>(P, o, cf);
            o.th = advance_heading(P, o.om, o.th);
            rotate_heading(o.om * P.h, o.c, o.s);
        }
        if (RSX_RARE_B(KIND, 1, is_ball && (o.z > 0.0f || o.vz > 0.0f))) ball_flight(P, o, K::e_ground, K::vz_min);   // the ball in flight
        // the position advance is the same instruction pair for robots and the ball, outside the role branches
        // (every role branch of a lane group costs a save / branch / restore of the exec mask; idle lanes hold zeros)
        o.x = fma_(o.vx, P.h, o.x);
        o.y = fma_(o.vy, P.h, o.y);
#ifdef RSX_TIMING_SUB
        ts1 = __builtin_readcyclecounter();
#endif

        // ---- B: contacts — one Jacobi sweep over the post-integration snapshot, and a second one
        // over the corrected snapshot for the envs in which some pair overlapped by more than pen2
        // (impacts at speed, jammed piles; resting contacts stay far below).  The second sweep is
        // the same loop body again: the instructions are in the cache (a separate copy never is) ----
        // is the env's ball low enough to be touched?  One ballot of the ball lanes' answer, each lane picks its env's bit
        // (was: the height through LDS — a write, a dependent read and its wait in every sub-step)
        const unsigned long long lowm = __ballot(is_ball && o.z < K::robot_h);
        bool ball_low = ((lowm >> (LaneMap<L>::slot(N, g))) & 1ull) != 0;
        bool active = is_robot || is_ball;   // lanes whose env takes part in the current sweep
        BallOverride bo{false, false, 0.0f, 0.0f, 0.0f};
        for (int sweep = 0;; ++sweep) {
            float2 fo = float2{0.0f, 0.0f};   // VSS: this body's held axes in the snapshot of this sweep (robots; the ball publishes zeros)
            if (active) {
                sh.A[lane] = make_float4(o.x, o.y, o.vx, o.vy);
                sh.W[lane] = o.om;   // yaw rate / spin: read on the contact path only
                sh.X[g * L + b] = o.x; sh.Y[g * L + b] = o.y;
            }
            wave_sync();
            // VSS: the held axes of this snapshot are computed and published BEHIND the exchange — the arithmetic fills the wait for the
            // partners' positions (overlap_keys_packed: `fill`).  Read on the contact path only; no second exchange point is needed: a
            // wave's LDS accesses execute in issue order, and the compiler keeps this write ahead of the later reads of the same array
            // (they may alias).  (A wave_sync() at the head of the contact branch was measured: it pins the body's position in scratch
            // memory, 8.9 -> 12.8 us.)
            auto publish_held = [&]() {
                if constexpr (K::held) { fo = held_axes<KIND>(P, o.x, o.y, is_robot); sh.F[lane] = fo; }
            };
            bool deep = false;   // this lane saw a deep contact
            bool wallp = false;  // ... a touching robot - robot pair with a wall-blocked axis (model v2: wall_shares)

            if (KIND == RSX_KIND_VSS) {
                // every pair is circle-circle; only the constants depend on the pair type
                if (active) {
                    if (NR) {
                        // Overlap test of the whole sweep, exact and with ONE compare per partner class:
                        // d2 is a sum of squares (>= +0), and non-negative floats order like their bit
                        // patterns, so with u = bits(d2) - 1 (d2 == 0, the lane's own slot, wraps to
                        // 0xFFFFFFFF)   0 < d2 < thr   <=>   u < bits(thr) - 1   (unsigned).
                        // The minimum of u over the robot slots is compared once; contacts are rare, so
                        // the common case is ~5 instructions per partner and one untaken branch.
                        constexpr uint32_t T_RR = __builtin_bit_cast(uint32_t, K::rs_rr2) - 1u;
                        constexpr uint32_t T_RB = __builtin_bit_cast(uint32_t, K::rs_rb2) - 1u;
                        uint32_t u[NR + 1];
                        if constexpr (K::held) overlap_keys_packed<NR + 1, L>(sh, g, o.x, o.y, u, publish_held);
                        else overlap_keys_packed<NR + 1, L>(sh, g, o.x, o.y, u);
                        uint32_t um = u[0];
#pragma unroll
                        for (int j = 1; j < NR; ++j) um = min(um, u[j]);
                        // robot lane: robot slots are robot-robot pairs, slot NR the ball; ball lane:
                        // every robot slot is a robot-ball pair, slot NR itself (u = 0xFFFFFFFF)
                        const bool any = ((um < (is_ball ? T_RB : T_RR)) & (!is_ball | ball_low)) | ((u[NR] < T_RB) & ball_low);
                        if (RSX_RARE_B(KIND, 2, any)) {
                            // Each lane walks ITS partners in body-index order; lanes with different
                            // partners share an iteration, so a wave pays for the deepest lane (one
                            // response, rarely two) instead of one response block per distinct partner
                            // index present anywhere in the wave.  The wave that finishes last sets a
                            // single-step launch's duration, and it is always one with contacts.
                            // slot j ends at bit j: shifted in from the right, highest slot first — a compare and an add-with-
                            // carry per slot, no bit constant in a register; the ball's height gates its pairs afterwards
                            unsigned todo = 0;
                            const uint32_t thr_r = is_ball ? T_RB : T_RR;   // robot slots: robot-ball pairs for the ball lane
#pragma unroll
                            for (int j = NR; j >= 0; --j) {
                                if (j == NR) asm("v_cmp_gt_u32_e32 vcc, %2, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc" : "+v"(todo) : "v"(u[j]), "s"(T_RB) : "vcc");
                                else asm("v_cmp_gt_u32_e32 vcc, %2, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc" : "+v"(todo) : "v"(u[j]), "v"(thr_r) : "vcc");
                            }
                            if (!ball_low) todo = is_ball ? 0u : (todo & ~(1u << NR));
                            const bool v2w = K::wall_aware && __ballot(is_robot && at_wall<KIND>(P, o.x, o.y)) != 0ull;   // (rsx_body.hpp: contact_response)
                            float avx = 0.0f, avy = 0.0f, apx = 0.0f, apy = 0.0f, aw = 0.0f;
                            const float lever = is_ball ? K::r_ball : K::r_robot;
                            // software-pipelined: the next partner's slot is fetched while the current
                            // response is being computed
                            int jn = __builtin_ctz(todo);
                            todo &= todo - 1;
                            float4 nxt = sh.A[LaneMap<L>::slot(jn, g)];
                            float nxw = sh.W[LaneMap<L>::slot(jn, g)];
                            float2 nxf = sh.F[LaneMap<L>::slot(jn, g)];
                            for (;;) {
                                const int j = jn;
                                const float4 oj = nxt;
                                const float wj = nxw;
                                const float2 fj = nxf;
                                const bool more = todo != 0;
                                if (more) {
                                    jn = __builtin_ctz(todo);
                                    todo &= todo - 1;
                                    nxt = sh.A[LaneMap<L>::slot(jn, g)];
                                    nxw = sh.W[LaneMap<L>::slot(jn, g)];
                                    nxf = sh.F[LaneMap<L>::slot(jn, g)];
                                }
                                const float dx = oj.x - o.x, dy = oj.y - o.y;
                                const float d2 = fma_(dx, dx, dy * dy);   // the value the sweep above saw
                                const bool rb = is_ball || j == NR;
                                contact_response<KIND>(P, o, oj, d2, rb ? K::rs_rb : K::rs_rr, rb ? cf.ope_rb() : cf.ope_rr(),
                                                       is_ball ? cf.w_rb_b() : (j == NR ? cf.w_rb_r() : K::w_rr),
                                                       is_ball ? cf.kt_rb_b() : (j == NR ? cf.kt_rb_r() : K::kt_rr),
                                                       rb ? cf.mu_rb() : cf.mu_rr(), is_ball ? K::spin_c : 0.0f,
                                                       fma_(wj, j == NR ? K::r_ball : K::r_robot, o.om * lever), K::beta, K::pen2, !rb, v2w,
                                                       avx, avy, apx, apy, aw, deep, wallp, fo, fj);
                                if (!more) break;
                            }
                            // only a body that touched something is updated (the others keep their bits)
                            o.vx = o.vx + avx; o.vy = o.vy + avy;
                            o.x = o.x + apx; o.y = o.y + apy;
                            if (is_ball) o.om = o.om + aw;
                        }
                    } else {
                        publish_held();
                        deep = vss_sweep_loop<KIND, L>(P, o, N, g, is_ball, ball_low, sh, wallp, fo, cf);
                    }
                }
            } else {
                deep = ssl_sweep<KIND, L, NR>(P, o, N, g, lane, is_robot && active, is_ball && active, ball_low, sweep == 0, sh, bo, wallp, cf);
            }
            // second sweep for the envs in which some pair was deep: one ballot, usually no lane; a third and a fourth one for the
            // envs in which the last sweep also saw a wall pair (model v2: piles pressed against a wall)
            const unsigned long long dmask = __ballot(deep);
            if (sweep == 3 || !RSX_RARE_B(KIND, 2, dmask != 0)) break;
            bool again = (L == 64 ? dmask : (dmask & env_lane_mask<L>(g))) != 0;
            if (sweep >= 1) {
                const unsigned long long wmask = __ballot(wallp);
                again = again && (L == 64 ? wmask : (wmask & env_lane_mask<L>(g))) != 0;
            }
            active = active && again;
            if (sweep >= 1 && !__any(active)) break;
            wave_sync();   // every lane has read the first snapshot before it is republished
        }
        if (KIND == RSX_KIND_SSL && bo.ovr) {   // kicker / dribbler: decided in the first sweep, applied after the impulses
            o.vx = bo.ovx; o.vy = bo.ovy; o.om = 0.0f;
            if (bo.okick && bo.ovz > 0.0f) o.vz = bo.ovz;
        }

        // ---- C: walls ----
        // SSL: every lane, no role branch (idle lanes hold zeros: inside every wall) — measured 1-3 % on the SSL tasks;
        // the VSS-v0 3v3 single-step kernel measured 1.5 % slower that way and keeps the branch
        // (SSL also: only when some body of the wave is near a wall — near_walls, rsx_body.hpp: the clamp is the identity elsewhere)
#ifdef RSX_TIMING_SUB
        ts2 = __builtin_readcyclecounter();
#endif
        if (KIND == RSX_KIND_SSL ? __any(near_walls<KIND>(P, o.x, o.y)) : (is_robot || is_ball)) {
            const float vx0 = o.vx, vy0 = o.vy;
            int hit = 0;
            if constexpr (KIND == RSX_KIND_VSS) {
                // the goal-post response shares the rare branch of the ball's wall friction (one exec-mask branch at the end of every
                // sub-step instead of two: a lone wave pays for each one's compare -> scalar -> branch chain)
                const float rb = is_ball ? K::r_ball : K::r_robot, eb = is_ball ? cf.e_wb() : cf.e_wr();
                walls<KIND, true>(P, rb, eb, o.x, o.y, o.vx, o.vy, hit);
                if (RSX_RARE_B(KIND, 2, (is_ball && (hit & 3)) || (hit & 8))) {
                    if (hit & 8) post_response(P, rb, eb, o.x, o.y, o.vx, o.vy, hit);
                    if (is_ball && (hit & 3)) ball_wall_spin<KIND>(hit, vx0, vy0, o.vx, o.vy, o.om, cf.mu_wb(), cf.ope_wb());
                }
            } else {
            walls<KIND>(P, is_ball ? K::r_ball : K::r_robot, is_ball ? cf.e_wb() : cf.e_wr(), o.x, o.y, o.vx, o.vy, hit);
            if (RSX_RARE_B(KIND, 2, is_ball && hit)) ball_wall_spin<KIND>(hit, vx0, vy0, o.vx, o.vy, o.om, cf.mu_wb(), cf.ope_wb());
            }
        }
        wave_sync();  // A / W / Bq / Cq / Dq are rewritten by the next sub-step
#ifdef RSX_TIMING
        if (threadIdx.x == 0 && sh.dbg) sh.dbg[(size_t)(8 + sub) * gridDim.x + blockIdx.x] = __builtin_readcyclecounter();
#endif
#ifdef RSX_TIMING_SUB
        if (sub >= 1) { const unsigned long long t3 = __builtin_readcyclecounter(); tsA += ts1 - ts0; tsB += ts2 - ts1; tsC += t3 - ts2; }
#endif
    }
#ifdef RSX_TIMING_SUB
    if (threadIdx.x == 0 && sh.dbg) {
        sh.dbg[(size_t)15 * gridDim.x + blockIdx.x] = tsA; sh.dbg[(size_t)16 * gridDim.x + blockIdx.x] = tsB; sh.dbg[(size_t)17 * gridDim.x + blockIdx.x] = tsC;
    }
#endif
}

}  // namespace rsx
