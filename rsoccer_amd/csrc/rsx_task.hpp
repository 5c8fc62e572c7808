// rsx_task.hpp — what a task means, stated once for every kernel layout: observation entries (write_obs) and their
// compile-time width (obs_dim_c), actions -> robot commands (vss_wheel, ssl_agent_commands), reward / termination / info
// terms (task_reward) and the random numbers of a step (draw_for_step).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsx_math.hpp"
#include "rsx_params.hpp"

namespace rsx {

// observation width: a compile-time constant when the team sizes are (lets the copy-out unroll); 0 = run-time (Params::obs_dim)
template <int TASK, int NR>
constexpr int obs_dim_c() {
    return NR == 0 ? 0
        : TASK == RSX_TASK_VSS_V0 ? 4 + 6 * NR                // equal teams: 4 + 7*nb + 5*ny (vss_gym.py:64-67): 40 for 3v3, 64 for 5v5
        : TASK == RSX_TASK_SSL_STATIC_DEFENDERS ? 4 + 8 + 2 * (NR - 1)
        : TASK == RSX_TASK_SSL_SCRIMMAGE ? 2 + 2 * NR
        : TASK == RSX_TASK_SSL_DRIBBLING ? 21 : TASK == RSX_TASK_SSL_CONTESTED ? 14 : 16;
}

// observation entries owned by this lane -> staging row of its env; values are the WIRE-format
// state.  Layouts: vss_gym.py:93-117, static_defenders.py:90-112, dribbling.py:76-104,
// contested_possession.py:78-104, pass_endurance.py:77-91.
// nb = blue robots (run-time for the lanes kernels, a constant for the one-lane-per-env kernels, whose
// "row" is a register array)
template <int KIND, int TASK>
__device__ __forceinline__ void write_obs_nb(const Params& P, float* __restrict__ row, int b, const int nb,
                                             bool is_robot, bool is_ball, float x, float y, float vx,
                                             float vy, float sn, float cs, float om_deg, int ir,
                                             float tscalar) {
    // sn / cs = sin / cos of (theta_deg * deg2rad), i.e. of the wire-format heading
    using T = TC<TASK>;
    const float lo = -1.2f, hi = 1.2f;
    if (TASK == RSX_TASK_SSL_SCRIMMAGE) {   // positions only (README.md:88-90 style)
        if (is_ball || is_robot) {
            float* r = row + (is_ball ? 0 : 2 + 2 * b);
            r[0] = clampf(x * P.inv_max_pos, lo, hi);
            r[1] = clampf(y * P.inv_max_pos, lo, hi);
        }
        return;
    }
    constexpr int OFF = TASK == RSX_TASK_SSL_DRIBBLING ? 1 : 0;   // dribbling: slot 0 = checkpoint progress
    constexpr int WB = TASK == RSX_TASK_VSS_V0 ? 7 : (TASK == RSX_TASK_SSL_PASS_ENDURANCE ? 6 : 8);
    constexpr int WY = TASK == RSX_TASK_VSS_V0 ? 5 : 2;
    if (is_ball) {
        if (OFF) row[0] = ((tscalar / 6.0f) * 2.0f) - 1.0f;
        row[OFF + 0] = clampf(x * P.inv_max_pos, lo, hi);
        row[OFF + 1] = clampf(y * P.inv_max_pos, lo, hi);
        row[OFF + 2] = clampf(vx * T::inv_max_v, lo, hi);
        row[OFF + 3] = clampf(vy * T::inv_max_v, lo, hi);
    } else if (is_robot) {
        if (b < nb) {
            float* r = row + OFF + 4 + WB * b;
            r[0] = clampf(x * P.inv_max_pos, lo, hi);
            r[1] = clampf(y * P.inv_max_pos, lo, hi);
            r[2] = sn; r[3] = cs;
            if (TASK == RSX_TASK_SSL_PASS_ENDURANCE) {
                r[4] = clampf(om_deg * T::inv_max_w, lo, hi);
                r[5] = ir ? 1.0f : 0.0f;
            } else {
                r[4] = clampf(vx * T::inv_max_v, lo, hi);
                r[5] = clampf(vy * T::inv_max_v, lo, hi);
                r[6] = clampf(om_deg * T::inv_max_w, lo, hi);
                if (TASK == RSX_TASK_SSL_DRIBBLING) r[7] = ir ? 1.0f : -1.0f;
                else if (TASK != RSX_TASK_VSS_V0) r[7] = ir ? 1.0f : 0.0f;
            }
        } else {
            float* r = row + OFF + 4 + WB * nb + WY * (b - nb);
            r[0] = clampf(x * P.inv_max_pos, lo, hi);
            r[1] = clampf(y * P.inv_max_pos, lo, hi);
            if (TASK == RSX_TASK_VSS_V0) {
                r[2] = clampf(vx * T::inv_max_v, lo, hi);
                r[3] = clampf(vy * T::inv_max_v, lo, hi);
                r[4] = clampf(om_deg * T::inv_max_w, lo, hi);
            }
        }
    }
}

template <int KIND, int TASK>
__device__ __forceinline__ void write_obs(const Params& P, float* __restrict__ row, int b,
                                          bool is_robot, bool is_ball, float x, float y, float vx,
                                          float vy, float sn, float cs, float om_deg, int ir,
                                          float tscalar) {
    write_obs_nb<KIND, TASK>(P, row, b, P.n_blue, is_robot, is_ball, x, y, vx, vy, sn, cs, om_deg, ir, tscalar);
}

// Return of a finished VSS-v0 episode, from its cumulative reward terms (vss_gym.py:151-158,186-190):
// shaping sums + 10 per goal for, -10 per goal against.  (No running sum of rewards is kept.)
__device__ __forceinline__ float vss_episode_return(const float* info) {
    return ((info[1] + info[2]) + info[3]) + 10.0f * info[0];
}

// vss_gym.py:235-254
__device__ __forceinline__ float vss_wheel(float a) {
    using T = TC<RSX_TASK_VSS_V0>;
    using K = KC<RSX_KIND_VSS>;
    float v = a * T::max_v;
    v = clampf(v, -T::max_v, T::max_v);
    if (-T::deadzone < v && v < T::deadzone) v = 0.0f;
    return v * K::inv_rw;
}

// Action of the agent (blue 0) of an SSL task -> its robot command q (robosim order: wheel speeds flag,
// v_x, v_y, v_theta, kick_x, kick_z is q[5]..., dribbler q[7]); (sn, cs) = sine and cosine of the robot's heading: the
// body's own (s, c), which every step start and end derive from the stored heading in degrees by sincos_f32 — the
// reference evaluates sin / cos of that same float (static_defenders.py:128-131).
template <int TASK>
__device__ __forceinline__ void ssl_agent_commands(const float* a, const float sn, const float cs, float* q) {
    using K = KC<RSX_KIND_SSL>;
    using T = TC<TASK>;
    if (TASK == RSX_TASK_SSL_PASS_ENDURANCE) {  // pass_endurance.py:106-130
        float k = fabsf(a[1]) > 0.5f ? a[1] : 0.0f;
        q[3] = a[0] * 10.0f;
        q[5] = k * 5.0f;
        q[7] = a[2] > 0.0f ? 1.0f : 0.0f;
    } else {  // static_defenders.py:114-148, dribbling.py:106-135, contested_possession.py:106-137
        float gx = a[0] * T::max_v, gy = a[1] * T::max_v, vth = a[2] * 10.0f;
        float lx = gx * cs + gy * sn, ly = gy * cs - gx * sn;
        float nrm = sqrtf(lx * lx + ly * ly);
        if (!(nrm < T::max_v)) { float sc = T::max_v / nrm; lx = lx * sc; ly = ly * sc; }
        q[1] = lx; q[2] = ly; q[3] = vth;
        if (TASK == RSX_TASK_SSL_DRIBBLING) {
            q[7] = a[3] > 0.0f ? 1.0f : 0.0f;
        } else {
            q[5] = a[3] > 0.0f ? 5.0f : 0.0f;
            q[7] = a[4] > 0.0f ? 1.0f : 0.0f;
        }
    }
}

// Reward, termination and info terms of one env step, from the post-step ball position (bx, by), the
// pre-step one (lastx, lasty) and xr[] = what the task needs from the robots (filled by the caller: see
// task_step_kernel).  One body for both tile layouts, so their arithmetic cannot drift apart.
template <int KIND, int TASK>
__device__ __forceinline__ void task_reward(const Params& P, const float* xr, const float bx, const float by,
                                            const float lastx, const float lasty, const bool first_step,
                                            float& prev_pot, float* info, float& reward, int& term,
                                            bool& success, bool& against) {
    using T = TC<TASK>;
    reward = 0.0f; term = 0;
    if (TASK == RSX_TASK_VSS_V0) {  // vss_gym.py:144-192,256-311
        if (bx > P.half_len) { info[0] += 1.0f; info[4] += 1.0f; reward = 10.0f; term = 1; }
        else if (bx < -P.half_len) { info[0] -= 1.0f; info[5] += 1.0f; reward = -10.0f; term = 1; }
        else {
            float pot = vss_ball_potential(bx, by, P.hl_goal, P.inv_len_cm);
            float grad = 0.0f;
            if (!first_step) grad = clampf((pot - prev_pot) * 3.0f * P.inv_dt, -5.0f, 5.0f);
            prev_pot = pot;
            float rbx = bx - xr[0], rby = by - xr[1];
            float nrm = sqrtf(rbx * rbx + rby * rby);
            float mv = nrm > 0.0f ? (rbx / nrm) * xr[2] + (rby / nrm) * xr[3] : 0.0f;   // unguarded in vss_gym.py:298
            float move = clampf(mv * 2.5f, -5.0f, 5.0f);
            float energy = -(fabsf(xr[4]) + fabsf(xr[5]));
            float t_move = 0.2f * move, t_grad = 0.8f * grad, t_en = 2e-4f * energy;
            reward = (t_move + t_grad) + t_en;
            info[1] += t_move; info[2] += t_grad; info[3] += t_en;
        }
    } else if (TASK == RSX_TASK_SSL_SCRIMMAGE) {  // README.md:96-102 style: a goal ends the episode
        if (bx > P.half_len && fabsf(by) < P.ghw) { reward = 1.0f; term = 1; info[0] += 1.0f; }
        else if (bx < -P.half_len && fabsf(by) < P.ghw) { reward = -1.0f; term = 1; info[1] += 1.0f; }
        success = info[0] > 0.0f; against = info[1] > 0.0f;
    } else if (TASK == RSX_TASK_SSL_DRIBBLING) {  // dribbling.py:137-185; prev_pot = checkpoints_count
        const float rx = xr[0], ry = xr[1];
        if (xr[2] != 0.0f || xr[3] != 0.0f || xr[4] != 0.0f || xr[5] != 0.0f) term = 1;  // an obstacle was hit
        if (rx < -3.0f || rx > 1.0f || fabsf(ry) > 1.0f) term = 1;                         // left the course
        else {
            const int n = (int)prev_pot;
            const bool down = lasty >= 0.0f && by < 0.0f, up = lasty < 0.0f && by >= 0.0f;
            bool passed;
            if (n == 0) passed = bx < -0.5f && bx > -1.0f && down;
            else if (n == 1) passed = bx < -1.0f && bx > -1.5f && up;
            else if (n % 2 == 0) {
                const bool inside = bx < -1.5f && bx > -2.0f;
                passed = inside && down;
                if (inside && !down && up) term = 1;   // reversed the last checkpoint
            } else passed = bx > -3.0f && bx < -2.0f && up;
            if (passed) {
                reward = 1.0f;
                prev_pot = (float)(n + 1);
                if (n >= 2 && n % 2 == 0 && n + 1 == 7) term = 1;   // course completed
            }
        }
        info[0] = prev_pot;
        success = prev_pot >= 7.0f;
    } else if (TASK == RSX_TASK_SSL_PASS_ENDURANCE) {  // pass_endurance.py:132-154,187-233; prev_pot = stopped_steps
        const float shx = xr[0], shy = xr[1], rcx = xr[2], rcy = xr[3];
        const bool rc_ir = xr[4] != 0.0f;
        float ddx = rcx - bx, ddy = rcy - by, ldx = rcx - lastx, ldy = rcy - lasty;
        float dist = sqrtf(ddx * ddx + ddy * ddy), last_dist = sqrtf(ldx * ldx + ldy * ldy);
        if (rc_ir) { reward = 1.0f; term = 1; }
        else {
            float gr = P.inv_bg_scale * clampf(last_dist - dist, -1.0f, 1.0f);
            reward = gr; info[1] += gr;
        }
        // "wrong ball": outside the shooter-receiver box on a centimetre grid, or stalled
        const int cbx = (int)(bx * 100.0f), cby = (int)(by * 100.0f);
        const int csx = (int)(shx * 100.0f), csy = (int)(shy * 100.0f);
        const int crx = (int)(rcx * 100.0f), cry = (int)(rcy * 100.0f);
        const bool in_x = min(crx, csx) <= cbx && cbx <= max(crx, csx);
        const bool in_y = min(cry, csy) <= cby && cby <= max(cry, csy);
        if (fabsf(last_dist - dist) < 0.01f) prev_pot = prev_pot + 1.0f; else prev_pot = 0.0f;
        if (prev_pot > 20.0f || !(in_x && in_y)) { reward = reward - 1.0f; term = 1; }
        if (term) {
            float rdx = rcx - shx, rdy = rcy - shy;
            float dist_robs = sqrtf(rdx * rdx + rdy * rdy);
            info[0] = dist_robs > 0.0f ? (dist_robs - dist) / dist_robs : 0.0f;
        }
        success = term && rc_ir;
    } else {  // static_defenders.py:150-212,256-322; contested_possession.py:139-201
        const float rx = xr[0], ry = xr[1];
        if (TASK == RSX_TASK_SSL_CONTESTED && xr[2] != 0.0f) { info[8] += 1.0f; term = 1; }  // opponent moved
        if (rx < -0.2f || fabsf(ry) > P.half_wid) { term = 1; info[4] += 1.0f; }
        else if (rx > P.pen_x && fabsf(ry) < P.half_pen_wid) { term = 1; info[1] += 1.0f; }
        else if (bx < 0.0f || fabsf(by) > P.half_wid) { term = 1; info[2] += 1.0f; }
        else if (bx > P.half_len) {
            term = 1;
            if (fabsf(by) < P.ghw) { reward = 5.0f; info[0] += 1.0f; }
            else info[3] += 1.0f;
        } else {
            float ldx = xr[6] - lastx, ldy = xr[7] - lasty;
            float cdx = rx - bx, cdy = ry - by;
            float bd = clampf(sqrtf(ldx * ldx + ldy * ldy) - sqrtf(cdx * cdx + cdy * cdy), -1.0f, 1.0f) * P.inv_bd_scale;
            float lgx = P.half_len - lastx, cgx = P.half_len - bx;
            float bg = clampf(sqrtf(lgx * lgx + lasty * lasty) - sqrtf(cgx * cgx + by * by), -1.0f, 1.0f) * P.inv_bg_scale;
            float en = -(((fabsf(xr[8]) + fabsf(xr[9])) + fabsf(xr[10])) + fabsf(xr[11])) * T::inv_en_scale;
            info[5] += bd; info[6] += bg; info[7] += en;
            reward = (bd + bg) + en;
        }
        success = info[0] > 0.0f;
    }
}

// The random numbers of one step for the body of this lane.  They depend on (seed, global env id,
// handle step count) only — not on anything in memory — so a single-step launch computes them while
// its state loads are in flight (Philox + Box-Muller: ~1.5 k cycles that used to follow the ~1.8 k
// cycle load wait).  VSS-v0: robot 0 -> two uniforms in [-1, 1) (its random action), robots >= 1 ->
// two standard normals (Box-Muller, Utils/Utils.py:18); scrimmage: four uniforms per robot; the other
// SSL tasks: up to five uniforms for robot 0.
struct StepDraw { float v[5]; };

template <int KIND, int TASK>
__device__ __forceinline__ StepDraw draw_for_step(const Params& P, const uint32_t env_id, const uint32_t t,
                                                  const int b, const bool is_robot, const bool fed) {
    StepDraw d;
#pragma unroll
    for (int i = 0; i < 5; ++i) d.v[i] = 0.0f;
    if (TASK == RSX_TASK_VSS_V0) {
        if (is_robot && !(fed && b == 0)) {
            // one Philox call per lane: block b >> 1 of the step, this robot's pair of words
            const u32x4 u = philox4x32(env_id, 0u, t, DOM_ACT | ((uint32_t)(b >> 1) << 8), P.key0, P.key1);
            const uint32_t w0 = (b & 1) ? u.z : u.x, w1 = (b & 1) ? u.w : u.y;
            if (b == 0) { d.v[0] = u01(w0) * 2.0f - 1.0f; d.v[1] = u01(w1) * 2.0f - 1.0f; }
            else {
                float u1 = (float)((w0 >> 8) + 1u) * 5.9604644775390625e-08f;
                float ang = (u01(w1) - 0.5f) * 6.283185307179586f;
                float rad = sqrtf(-2.0f * log_f32(u1));
                float sn, cs;
                sincos_f32(ang, sn, cs);
                d.v[0] = rad * cs; d.v[1] = rad * sn;
            }
        }
    } else if (TASK == RSX_TASK_SSL_SCRIMMAGE) {
        if (is_robot && !fed) {
            const u32x4 u = philox4x32(env_id, 0u, t, DOM_ACT | ((uint32_t)b << 8), P.key0, P.key1);
            d.v[0] = u01(u.x) * 2.0f - 1.0f; d.v[1] = u01(u.y) * 2.0f - 1.0f;
            d.v[2] = u01(u.z) * 2.0f - 1.0f; d.v[3] = u01(u.w) * 2.0f - 1.0f;
        }
    } else {
        if (is_robot && b == 0 && !fed) {
            const u32x4 u = philox4x32(env_id, 0u, t, DOM_ACT, P.key0, P.key1);
            d.v[0] = u01(u.x) * 2.0f - 1.0f; d.v[1] = u01(u.y) * 2.0f - 1.0f;
            d.v[2] = u01(u.z) * 2.0f - 1.0f; d.v[3] = u01(u.w) * 2.0f - 1.0f;
            // fifth component: the low bytes u01 leaves unused in x, y, z (one block per step)
            const uint32_t w = (u.x & 0xFFu) | ((u.y & 0xFFu) << 8) | ((u.z & 0xFFu) << 16);
            d.v[4] = u01(w << 8) * 2.0f - 1.0f;
        }
    }
    return d;
}

}  // namespace rsx
