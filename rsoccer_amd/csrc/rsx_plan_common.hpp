// rsx_plan_common.hpp — what the planning units (rsx_plan.hip, rsx_plan_sampled.hip) share: the launch arguments of the per-pair
// loop (rsx_plan_body.inc) and the candidate sampler of rsx_task_lookahead_sampled / rsx_plan_candidates / rsx_plan_update.
//
// The sampler (include/rsx.h has the definition): candidate k >= 1 of env g is the plan mean plus sigma times a standard normal that
// is a counter-based draw like every other random number of the engine — Philox keyed by what the draw is for, recomputed where it
// is needed, never stored.  The three kernels that need a candidate's action all go through plan_noise4 and plan_action below, so
// they compute the same floats from the same expressions (the units are built with -ffp-contract=off).
#pragma once
#include <stdint.h>

#include "rsx_math.hpp"

namespace rsx {

namespace {   // (kernel argument types of kernels with internal linkage: one copy per unit, as the kernels themselves)

struct PlanArgs {
    const float* state;      // the handle's state rows (read only)
    const float* aux;        // the handle's scalar arena (read only)
    const uint32_t* ticks;   // device-keyed handles: the step-counter slots (slot 0 is read, never written), else nullptr
    int n_cand, horizon;
    float gamma;
};

}  // namespace

// rsx_plan_sampler as the kernels take it.  nblk: blocks of four normals per segment = ceil(act_dim / 4)
struct PlanSampler {
    uint32_t k0, k1;   // sample_seed lo, hi: the Philox key
    float sigma;
    int hold, nblk;
};

// two standard normals from two Philox words: the Box-Muller of draw_for_step's OU branch (rsx_task.hpp), same expressions
__device__ __forceinline__ void plan_normal_pair(const uint32_t w0, const uint32_t w1, float& n0, float& n1) {
    float u1 = (float)((w0 >> 8) + 1u) * 5.9604644775390625e-08f;
    float ang = (u01(w1) - 0.5f) * 6.283185307179586f;
    float rad = sqrtf(-2.0f * log_f32(u1));
    float sn, cs;
    sincos_f32(ang, sn, cs);
    n0 = rad * cs; n1 = rad * sn;
}

// eps of block q (= segment * nblk + (component >> 2)) of candidate k of global env id g at step counter `tick`: four normals,
// component i takes n[i & 3]
__device__ __forceinline__ void plan_noise4(const PlanSampler& S, const uint32_t g, const uint32_t k, const uint32_t tick, const uint32_t q,
                                            float n[4]) {
    const u32x4 u = philox4x32(g, k, tick, DOM_PLAN | (q << 8), S.k0, S.k1);
    plan_normal_pair(u.x, u.y, n[0], n[1]);
    plan_normal_pair(u.z, u.w, n[2], n[3]);
}

// one action component of candidate k: candidate 0 is the unperturbed plan
__device__ __forceinline__ float plan_action(const float mean, const float sigma, const float eps, const bool perturbed) {
    return clampf(perturbed ? mean + sigma * eps : mean, -1.0f, 1.0f);
}
}  // namespace rsx
