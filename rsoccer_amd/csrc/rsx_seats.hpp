// rsx_seats.hpp — the mirror and seat helpers of VSS-v0 self-play as a kernel with two policy images uses them (include/rsx.h:
// rsx_task_collect_selfplay's mirrored observation, rsx_task_collect_team's seat map), stated once for the three units that use them:
// rsx_selfplay.hip (the mirrored row), rsx_teamplay.hip and rsx_match.hip (all of it).  The two collect units stated these helpers in
// their own text before; their kernels' device assembly is the same with this header as without (profiles/r21_seats_isa.txt).
// Float moves and negations only: nothing here rounds.
#pragma once
#include <hip/hip_runtime.h>

#include "rsx_policy_mlp.hpp"
#include "rsx_variants.hpp"

namespace rsx {

namespace {   // (device code of kernels with internal linkage: one copy per unit, as the kernels themselves)

// floats of an env's action slot and of one side's image: rsx_policy_mlp.hpp's image with a slot that holds every seat's two outputs
__host__ __device__ inline int action_pitch(const int n_blue) { const int n = round4(2 * n_blue); return n > 8 ? n : 8; }
__host__ __device__ inline int image_floats(const PolicyImage& m, const int G, const int AP) { return m.rows + 3 * G * m.xs + G * AP; }

// entry i of seat s's row is entry seat_ix(i, s) of the side's row: "own" slots 0 and s exchanged, everything else in place
__device__ __forceinline__ int seat_ix(const int i, const int s) {
    const int d = 7 * s;
    return (i >= 4 && i < 11) ? i + d : (i >= 4 + d && i < 11 + d) ? i - d : i;
}

// the exchange itself, by lanes 0 .. 6 of the env (a lane moves its own two floats: doing it twice puts the row back)
__device__ __forceinline__ void exchange_own(float* __restrict__ row, const int s, const int b) {
    if (b < 7) {
        float* const p = row + 4 + b;
        const float u = p[0], v = p[7 * s];
        p[0] = v; p[7 * s] = u;
    }
}

// the mirrored row: VSS-v0's observation with the team colours swapped and the field turned by 180 degrees ("own" slot i holds yellow i,
// "other" slot j blue j; positions, linear velocities, sine and cosine negated, the angular velocity unchanged)
__device__ __forceinline__ void write_obs_mirrored(const Params& P, float* __restrict__ row, const int b, const int nb, const bool is_robot,
                                                   const bool is_ball, const float x, const float y, const float vx, const float vy,
                                                   const float sn, const float cs, const float om_deg) {
    using T = TC<RSX_TASK_VSS_V0>;
    const float lo = -1.2f, hi = 1.2f;
    if (is_ball) {
        row[0] = -clampf(x * P.inv_max_pos, lo, hi);
        row[1] = -clampf(y * P.inv_max_pos, lo, hi);
        row[2] = -clampf(vx * T::inv_max_v, lo, hi);
        row[3] = -clampf(vy * T::inv_max_v, lo, hi);
    } else if (is_robot) {
        if (b >= nb) {   // yellow b - nb: an "own" slot
            float* r = row + 4 + 7 * (b - nb);
            r[0] = -clampf(x * P.inv_max_pos, lo, hi);
            r[1] = -clampf(y * P.inv_max_pos, lo, hi);
            r[2] = -sn; r[3] = -cs;
            r[4] = -clampf(vx * T::inv_max_v, lo, hi);
            r[5] = -clampf(vy * T::inv_max_v, lo, hi);
            r[6] = clampf(om_deg * T::inv_max_w, lo, hi);
        } else {         // blue b: an "other" slot (behind the nb = ny own slots)
            float* r = row + 4 + 7 * nb + 5 * b;
            r[0] = -clampf(x * P.inv_max_pos, lo, hi);
            r[1] = -clampf(y * P.inv_max_pos, lo, hi);
            r[2] = -clampf(vx * T::inv_max_v, lo, hi);
            r[3] = -clampf(vy * T::inv_max_v, lo, hi);
            r[4] = clampf(om_deg * T::inv_max_w, lo, hi);
        }
    }
}

}  // namespace

}  // namespace rsx
