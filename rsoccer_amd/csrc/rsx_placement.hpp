// rsx_placement.hpp — where the bodies of a new episode stand: the sequential placement of an env (place_env), the same by all
// lanes of the env together (place_env_parallel), the speculative draws both read (place_predraw) and the placement cache
// with its helper workgroups (pcache_rows, placement_helper).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsx_math.hpp"
#include "rsx_params.hpp"
#include "rsx_lane_map.hpp"

namespace rsx {

// Random placement of one env (vss_gym.py:194-233 / static_defenders.py:214-254 with Philox
// draws).  The algorithm is sequential (every candidate is tested against the bodies already
// placed, and the index of a draw depends on how many were rejected before it), and runs on the
// env's ball lane; the expensive part, the Philox blocks, is hoisted: draws 0..NPRE-1 were
// computed speculatively by all lanes of the env (place_predraw) and are only read here.
// Poses go to A[body slot] = (x, y, theta_deg, 0).
// how many placement draws are computed ahead by the env's lanes: the rejection-sampled tasks
// use >= 13 (VSS-v0) / >= 15 (static defenders), pass endurance two plus its rejections (about
// half of its candidates; measured faster with the full block than with 4 or 8); contested
// possession uses exactly one, dribbling none (fixed course).  Later draws are computed where
// they are needed.
template <int TASK, int L>
__host__ __device__ constexpr int predraw_count() {
    return (TASK == RSX_TASK_SSL_DRIBBLING || TASK == RSX_TASK_SSL_SCRIMMAGE) ? 0 : TASK == RSX_TASK_SSL_CONTESTED ? 1 : (L < 16 ? 16 : L);
}

template <int TASK, int L>
__device__ __forceinline__ void place_predraw(const Params& P, uint32_t env_id, uint32_t episode,
                                              int b, float2* __restrict__ draws) {
    constexpr int NPRE = predraw_count<TASK, L>();
#pragma unroll
    for (int n = b; n < NPRE; n += L) {
        const u32x4 u = philox4x32(env_id, episode, (uint32_t)n, DOM_PLACE, P.key0, P.key1);
        draws[n] = make_float2(u01(u.x), u01(u.y));
    }
}

template <int TASK, int L, bool PRE = true>
__device__ __forceinline__ void place_env(const Params& P, const int N, uint32_t env_id,
                                          uint32_t episode, int g, float4* A, const float2* draws) {
    constexpr int G = 64 / L;
    constexpr int NPRE = PRE ? predraw_count<TASK, L>() : 0;   // !PRE: every draw is computed where it is used
    uint32_t n = 0;
    auto draw = [&]() -> float2 {
        const uint32_t i = n++;
        if (i < (uint32_t)NPRE) return draws[i];
        const u32x4 u = philox4x32(env_id, episode, i, DOM_PLACE, P.key0, P.key1);
        return make_float2(u01(u.x), u01(u.y));
    };
    int first = 0;
    float bx, by;
    if (TASK == RSX_TASK_SSL_DRIBBLING) {  // dribbling.py:187-202: fixed course
        A[LaneMap<L>::slot(N, g)] = make_float4(-0.1f, 0.0f, 0.0f, 0.0f);
        A[LaneMap<L>::slot(0, g)] = make_float4(0.0f, 0.0f, 180.0f, 0.0f);
        for (int k = 1; k < 5; ++k) A[LaneMap<L>::slot(k, g)] = make_float4(-0.5f * (float)k, 0.0f, 180.0f, 0.0f);
        return;
    }
    if (TASK == RSX_TASK_SSL_CONTESTED) {  // contested_possession.py:203-220: the opponent holds the ball
        const float2 u = draw();
        const float ex = P.pl_xlo + P.pl_xspan * u.x, ey = P.pl_ylo + P.pl_yspan * u.y;
        A[LaneMap<L>::slot(N, g)] = make_float4(ex - 0.1f, ey, 0.0f, 0.0f);
        A[LaneMap<L>::slot(0, g)] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        A[LaneMap<L>::slot(1, g)] = make_float4(ex, ey, 180.0f, 0.0f);
        return;
    }
    if (TASK == RSX_TASK_SSL_PASS_ENDURANCE) {  // pass_endurance.py:156-185
        const float2 u = draw();
        const float px = -1.5f + 3.0f * u.x, py = 1.5f + -3.0f * u.y;
        const float side = py < 0.0f ? -1.0f : 1.0f;
        const float sx = px, sy = py + 0.115f * side;
        float rx = 0.0f;
        for (int t = 0; t < 64; ++t) {
            const float2 v = draw();
            rx = -1.5f + 3.0f * v.x;
            if (!(fabsf(rx - px) < 1.0f)) break;
        }
        const float ry = -py;
        A[LaneMap<L>::slot(N, g)] = make_float4(px, py, 0.0f, 0.0f);
        A[LaneMap<L>::slot(0, g)] = make_float4(sx, sy, side > 0.0f ? 270.0f : 90.0f, 0.0f);
        A[LaneMap<L>::slot(1, g)] = make_float4(rx, ry, (atan2_f32(ry - sy, rx - sx) + 3.14159265358979323846f) * KC<RSX_KIND_SSL>::rad2deg, 0.0f);
        return;
    }
    if (TASK == RSX_TASK_SSL_STATIC_DEFENDERS) {
        bx = 0.0f; by = 0.0f;
        for (int t = 0; t < 64; ++t) {
            const float2 u = draw();
            bx = P.pl_xlo + P.pl_xspan * u.x;
            by = P.pl_ylo + P.pl_yspan * u.y;
            if (!(bx > P.pen_x && fabsf(by) < P.half_pen_wid)) break;
        }
        A[LaneMap<L>::slot(0, g)] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // blue 0 at the origin
        first = 1;
    } else {
        const float2 u = draw();
        bx = P.pl_xlo + P.pl_xspan * u.x;
        by = P.pl_ylo + P.pl_yspan * u.y;
    }
    A[LaneMap<L>::slot(N, g)] = make_float4(bx, by, 0.0f, 0.0f);
    for (int k = first; k < N; ++k) {
        float x = 0.0f, y = 0.0f;
        for (int t = 0; t < 64; ++t) {
            const float2 u = draw();
            x = P.pl_xlo + P.pl_xspan * u.x;
            y = P.pl_ylo + P.pl_yspan * u.y;
            bool ok = true;
            {   // ball first, then (static defenders) blue 0, then the robots placed so far
                float dx = x - bx, dy = y - by;
                if (dx * dx + dy * dy < P.pl_min_d2) ok = false;
            }
            for (int q = 0; q < k; ++q) {
                const float4 pq = A[LaneMap<L>::slot(q, g)];
                float dx = x - pq.x, dy = y - pq.y;
                if (dx * dx + dy * dy < P.pl_min_d2) ok = false;
            }
            if (ok) break;
        }
        const float2 u = draw();
        A[LaneMap<L>::slot(k, g)] = make_float4(x, y, 360.0f * u.x, 0.0f);
    }
}

// The same placement, run by all lanes of the env together (VSS-v0 and static defenders, whose
// placements are rejection loops).  The sequential algorithm consumes draws in order, so the
// draw index of robot k depends on how many candidates were rejected before it; here every
// robot k >= m (m = first robot not yet fixed) proposes its candidate ASSUMING no further
// rejection (draw n + 2(k-m) for the position, the next one for theta), each tests itself against
// the ball and all robots q < k (fixed or proposed), and the lowest failing robot f decides:
// m..f-1 were tested against accepted poses only, exactly as the sequential loop would have, and
// are fixed; f has used one more try and the draw indices behind it shift by one; robots > f
// propose again.  One round per rejection (+1) instead of ~2N dependent LDS round trips on a
// single lane; draws, candidates, tests and therefore results are those of place_env.
template <int TASK, int L, int NRC>
__device__ __forceinline__ float4 place_env_parallel(const Params& P, const int N, const uint32_t env_id,
                                                      const uint32_t episode, const int b, const int g,
                                                      const bool is_robot, float4* A, const float2* draws) {
    constexpr int G = 64 / L;
    constexpr int NPRE = predraw_count<TASK, L>();
    auto getdraw = [&](uint32_t i) -> float2 {
        if (i < (uint32_t)NPRE) return draws[i];
        const u32x4 u = philox4x32(env_id, episode, i, DOM_PLACE, P.key0, P.key1);
        return make_float2(u01(u.x), u01(u.y));
    };
    uint32_t n = 0;
    float bx = 0.0f, by = 0.0f;
    int m = 0;
    float x = 0.0f, y = 0.0f, th = 0.0f;   // this lane's robot
    if (TASK == RSX_TASK_SSL_STATIC_DEFENDERS) {
        for (int t = 0; t < 64; ++t) {
            const float2 u = getdraw(n++);
            bx = P.pl_xlo + P.pl_xspan * u.x;
            by = P.pl_ylo + P.pl_yspan * u.y;
            if (!(bx > P.pen_x && fabsf(by) < P.half_pen_wid)) break;
        }
        if (b == 0) A[LaneMap<L>::slot(0, g)] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // blue 0 at the origin
        m = 1;
    } else {
        const float2 u = getdraw(n++);
        bx = P.pl_xlo + P.pl_xspan * u.x;
        by = P.pl_ylo + P.pl_yspan * u.y;
    }
    // lanes of this env: body j sits at lane LaneMap<L>::slot(j, g)
    const unsigned long long envmask = env_lane_mask<L>(g);
    int t = 0;   // tries robot m has used
    while (m < N) {
        const bool spec = is_robot && b >= m;
        if (spec) {
            const uint32_t c = n + 2u * (uint32_t)(b - m);
            const float2 u = getdraw(c), v = getdraw(c + 1u);
            x = P.pl_xlo + P.pl_xspan * u.x;
            y = P.pl_ylo + P.pl_yspan * u.y;
            th = 360.0f * v.x;
            A[LaneMap<L>::slot(b, g)] = make_float4(x, y, th, 0.0f);
        }
        wave_sync();
        bool bad = false;
        if (spec) {
            {
                float dx = x - bx, dy = y - by;
                if (dx * dx + dy * dy < P.pl_min_d2) bad = true;
            }
            if (NRC) {
                float4 pq[NRC ? NRC : 1];
#pragma unroll
                for (int q = 0; q < NRC; ++q) pq[q] = A[LaneMap<L>::slot(q, g)];
#pragma unroll
                for (int q = 0; q < NRC; ++q) {
                    float dx = x - pq[q].x, dy = y - pq[q].y;
                    if ((q < b) & (dx * dx + dy * dy < P.pl_min_d2)) bad = true;
                }
            } else {
                for (int q = 0; q < b; ++q) {
                    const float4 pq = A[LaneMap<L>::slot(q, g)];
                    float dx = x - pq.x, dy = y - pq.y;
                    if (dx * dx + dy * dy < P.pl_min_d2) bad = true;
                }
            }
            if (b == m && t == 63) bad = false;   // the 64th candidate is taken as it is
        }
        wave_sync();   // the next round overwrites A
        const unsigned long long bm = __ballot(bad) & envmask;
        const int f = bm ? LaneMap<L>::body((int)__builtin_ctzll(bm)) : N;   // lowest failing robot
        if (f < N) {
            t = f == m ? t + 1 : 1;
            n += 2u * (uint32_t)(f - m) + 1u;
        }
        m = f;
    }
    return is_robot ? make_float4(x, y, th, 0.0f) : make_float4(bx, by, 0.0f, 0.0f);
}

// ---------------------------------------------------------------------------------------------
// Placement cache (single-step launches of SSLStaticDefenders 1v6 at latency-bound batch sizes).
//
// A single-step launch lasts as long as its slowest wave, and with short episodes that wave is one that resets an
// env: Philox blocks + rejection rounds are ~2.7 k cycles on top of a ~17 k cycle wave (1v6 at 2048 envs: 5.5 waves
// per launch hold a reset).  But the placement of an env's NEXT episode is a pure function of (seed, global env id,
// episode + 1): it can be computed at any time before it is needed, by anybody.  At these batches half of the chip's
// SIMDs are idle, so every step launch carries ceil(B / 64) extra HELPER workgroups behind the tile workgroups: helper
// w looks at envs [64 w, 64 w + 64) and, where the cached pose set is not the one of episode + 1, computes it with the
// same code the reset path runs (place_predraw + place_env_parallel: same draws, same tests, same poses) — eight envs
// at a time, far shorter than a step, never the slowest wave.  The resetting wave then only copies three floats per
// body that it loaded with its state.
//
// Two buffers, alternating by step parity: launch t writes buffer (t & 1) and reads buffer ((t + 1) & 1), which
// nobody writes during launch t — the only synchronisation is the kernel boundary.  An entry is tagged with the episode
// id it was made for; a tag that does not match (first steps after a reset, two episode ends in consecutive steps, a
// restored checkpoint) sends the env down the inline path, which stays as it was.  Layouts that do not use the cache
// ignore it: it is derived data, not state (not part of a checkpoint).
// Buffer: rows c * (N + 1) + b for c = x, y, theta and body b (ball = N), then the tag row; [rows][B] floats.
// ---------------------------------------------------------------------------------------------
template <int NB>
__host__ __device__ constexpr int pcache_rows() { return 3 * NB + 1; }

template <int KIND, int L, int TASK, int NR>
__device__ __forceinline__ void placement_helper(const Params& P, const Buffers& bufs, const int helper, const uint32_t tick, Shared<L>& sh) {
    static_assert(L == 8 && NR > 0, "the placement cache serves the 8-lane kernels of the fixed team sizes");
    constexpr int G = 64 / L, N = NR, NBD = N + 1;
    const size_t B = (size_t)P.num_envs;
    const int lane = threadIdx.x;
    const int b = LaneMap<L>::body(lane), g = LaneMap<L>::env(lane);
    float* const pw = bufs.pcache + (size_t)(tick & 1u) * (size_t)pcache_rows<NBD>() * B;
    // one lane per env: which of this wave's 64 envs lack the poses of their next episode?
    const int e0 = helper * 64 + lane;
    uint32_t ep_next = 0;
    bool stale = false;
    if (e0 < P.num_envs) {
        ep_next = __float_as_uint(bufs.aux[(size_t)ROW_EPISODE * (size_t)P.row_stride + e0]) + 1u;
        stale = __float_as_uint(pw[(size_t)(3 * NBD) * B + e0]) != ep_next;
    }
    unsigned long long todo = __ballot(stale);
    if (todo == 0) return;
    sh.ep[lane] = ep_next;
    wave_sync();
    while (todo) {   // eight envs per round: env slot g takes the g-th stale env
        unsigned long long mine = todo;
        for (int i = 0; i < g; ++i) mine &= mine - 1;
        const bool has = mine != 0;
        const int idx = has ? (int)__builtin_ctzll(mine) : 0;
        for (int i = 0; i < G && todo; ++i) todo &= todo - 1;
        const int e = helper * 64 + idx;
        const uint32_t env_id = P.env_id_base + (uint32_t)e;
        const uint32_t episode = sh.ep[idx];
        const bool is_robot = has && b < N, is_ball = has && b == N;
        if (has) place_predraw<TASK, L>(P, env_id, episode, b, sh.draws[g]);
        wave_sync();
        float4 pz = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (has) pz = place_env_parallel<TASK, L, NR>(P, N, env_id, episode, b, g, is_robot, sh.A, sh.draws[g]);
        if (is_robot || is_ball) {
            pw[(size_t)(0 * NBD + b) * B + e] = pz.x; pw[(size_t)(1 * NBD + b) * B + e] = pz.y; pw[(size_t)(2 * NBD + b) * B + e] = pz.z;
        }
        if (is_ball) pw[(size_t)(3 * NBD) * B + e] = __uint_as_float(episode);
        wave_sync();   // draws / A are rewritten by the next round
    }
}

}  // namespace rsx
