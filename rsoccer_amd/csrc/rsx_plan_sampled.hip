// rsx_plan_sampled.hip — planning with candidates that are never stored (include/rsx.h: rsx_task_lookahead_sampled,
// rsx_plan_candidates, rsx_plan_update), in a translation unit of its own so that the instantiations of every existing kernel stay
// exactly what they were.
//
// A candidate is the plan mean plus noise, and the noise is a counter-based draw (rsx_plan_common.hpp: plan_noise4, plan_action):
//   task_lookahead_sampled_kernel  task_lookahead_kernel (rsx_plan.hip) with each step's action drawn in registers instead of loaded:
//                                  the same per-pair loop (rsx_plan_body.inc), the same grid, the same outputs.  Only the lanes that
//                                  command a robot draw, once per segment of `hold` steps, one step ahead of the step that uses it —
//                                  where the loading kernel has its prefetch.
//   plan_candidates_kernel         writes those very actions out, [num_envs][K][H][act_dim]: elementwise, one thread per block of four
//   plan_update_kernel             folds [num_envs][K] returns into a new plan by drawing the candidates again: one thread per
//                                  (env, step, block of four components) walks the K candidates in index order
//
// plan_update_kernel's arithmetic is fixed: the best return is the first maximum in index order; weights are
// expf((R_k - R_best) / temperature) in float32; the weighted sums and the sum of weights are accumulated in float64 over k = 0, 1,
// ..., K - 1 by ONE thread (no atomics, no cross-lane reduction: nothing depends on the launch shape), divided in float64 and rounded
// once.  Each thread redraws K blocks: per (env, step) that is the work the lookahead spends per hold = 1 step on draws, without its physics.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rsx.h"
#include "rsx_plan_common.hpp"
#include "rsx_units.hpp"
#include "rsx_variants.hpp"

namespace rsx {

namespace {

template <int KIND, int TASK, int L, int NR, bool PHYS>
__global__ __launch_bounds__(64) void task_lookahead_sampled_kernel(const float* __restrict__ mean, float* __restrict__ returns,
                                                                    int32_t* __restrict__ steps_out, uint8_t* __restrict__ flags_out,
                                                                    float* __restrict__ last_obs, const int per_xcd, const Params P,
                                                                    const PlanArgs A, const PlanSampler S, const float* __restrict__ phys) {
// where a step's action comes from: the plan mean [num_envs][H][act_dim] (or zeros) plus this lane's noise, which is held for a
// segment and redrawn when STEP enters the next one.  Block of a lane: the robot's in the scrimmage (act_dim = 4 per robot), else
// component >> 2 of the agent's action
#define RSX_PLAN_ACT_SETUP                                                                                                            \
    const float* const my_mean = mean == nullptr ? nullptr                                                                            \
        : mean + (size_t)e * (size_t)A.horizon * step_floats + (TASK == RSX_TASK_SSL_SCRIMMAGE ? (size_t)b * AD : 0);                 \
    constexpr int NB = (AD + 3) / 4;                                                                                                  \
    float eps[4 * NB];                                                                                                                \
    _Pragma("unroll") for (int i = 0; i < 4 * NB; ++i) eps[i] = 0.0f;                                                                 \
    int seg = -1;
#define RSX_PLAN_ACT_FETCH(DST, STEP)                                                                                                 \
    {                                                                                                                                 \
        const int seg_of_step = (STEP) / S.hold;                                                                                      \
        if (k != 0 && seg_of_step != seg) {                                                                                           \
            _Pragma("unroll") for (int j = 0; j < NB; ++j)                                                                            \
                plan_noise4(S, env_id, (uint32_t)k, tick0,                                                                            \
                            (uint32_t)seg_of_step * (uint32_t)S.nblk + (uint32_t)(TASK == RSX_TASK_SSL_SCRIMMAGE ? b : j), eps + 4 * j); \
        }                                                                                                                             \
        seg = seg_of_step;                                                                                                            \
        _Pragma("unroll") for (int i = 0; i < AD; ++i)                                                                                \
            DST[i] = plan_action(my_mean ? my_mean[(size_t)(STEP) * step_floats + i] : 0.0f, S.sigma, eps[i], k != 0);                \
    }
#include "rsx_plan_body.inc"
#undef RSX_PLAN_ACT_SETUP
#undef RSX_PLAN_ACT_FETCH
}

// (env, candidate, step, block) of a flat index: the block fastest, as the output is laid out
struct PlanFlat {
    const float* mean;       // [num_envs][H][act_dim] or nullptr = zeros
    const uint32_t* ticks;   // as PlanArgs::ticks
    uint32_t tick_base, env_id_base;
    int num_envs, n_cand, horizon, act_dim;
};

__device__ __forceinline__ uint32_t plan_tick(const PlanFlat& F) { return F.ticks != nullptr ? F.ticks[0] : F.tick_base; }

__global__ __launch_bounds__(256) void plan_candidates_kernel(float* __restrict__ out, const PlanFlat F, const PlanSampler S) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)F.num_envs * (size_t)F.n_cand * (size_t)F.horizon * (size_t)S.nblk;
    if (idx >= total) return;
    const int j = (int)(idx % (size_t)S.nblk);
    size_t r = idx / (size_t)S.nblk;
    const int t = (int)(r % (size_t)F.horizon); r /= (size_t)F.horizon;
    const int k = (int)(r % (size_t)F.n_cand);
    const size_t e = r / (size_t)F.n_cand;
    float n[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (k != 0) plan_noise4(S, F.env_id_base + (uint32_t)e, (uint32_t)k, plan_tick(F), (uint32_t)(t / S.hold) * (uint32_t)S.nblk + (uint32_t)j, n);
    const size_t m_at = (e * (size_t)F.horizon + (size_t)t) * (size_t)F.act_dim;
    const size_t o_at = ((e * (size_t)F.n_cand + (size_t)k) * (size_t)F.horizon + (size_t)t) * (size_t)F.act_dim;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int i = 4 * j + c;
        if (i < F.act_dim) out[o_at + i] = plan_action(F.mean ? F.mean[m_at + i] : 0.0f, S.sigma, n[c], k != 0);
    }
}

// (mean and new_mean may be the same array: a thread reads its own four components before it writes them, and nobody else's)
__global__ __launch_bounds__(256) void plan_update_kernel(const float* __restrict__ returns, float* new_mean, int32_t* __restrict__ best_out,
                                                          const float temperature, const PlanFlat F, const PlanSampler S) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)F.num_envs * (size_t)F.horizon * (size_t)S.nblk;
    if (idx >= total) return;
    const int j = (int)(idx % (size_t)S.nblk);
    const size_t r = idx / (size_t)S.nblk;
    const int t = (int)(r % (size_t)F.horizon);
    const size_t e = r / (size_t)F.horizon;
    const float* const R = returns + e * (size_t)F.n_cand;
    // the best candidate: the first maximum in index order
    int best = 0;
    float r_best = R[0];
    for (int k = 1; k < F.n_cand; ++k) {
        const float rk = R[k];
        if (rk > r_best) { r_best = rk; best = k; }
    }
    if (t == 0 && j == 0 && best_out != nullptr) best_out[e] = best;
    const size_t m_at = (e * (size_t)F.horizon + (size_t)t) * (size_t)F.act_dim;
    float m[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) m[c] = (F.mean != nullptr && 4 * j + c < F.act_dim) ? F.mean[m_at + 4 * j + c] : 0.0f;
    const uint32_t g = F.env_id_base + (uint32_t)e, tick = plan_tick(F);
    const uint32_t q = (uint32_t)(t / S.hold) * (uint32_t)S.nblk + (uint32_t)j;
    float out[4];
    if (temperature == 0.0f) {   // the best candidate itself, bit for bit
        float n[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (best != 0) plan_noise4(S, g, (uint32_t)best, tick, q, n);
#pragma unroll
        for (int c = 0; c < 4; ++c) out[c] = plan_action(m[c], S.sigma, n[c], best != 0);
    } else {
        double acc[4] = {0.0, 0.0, 0.0, 0.0}, z = 0.0;
        for (int k = 0; k < F.n_cand; ++k) {
            const float w = expf((R[k] - r_best) / temperature);
            float n[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (k != 0) plan_noise4(S, g, (uint32_t)k, tick, q, n);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = acc[c] + (double)w * (double)plan_action(m[c], S.sigma, n[c], k != 0);
            z = z + (double)w;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) out[c] = (float)(acc[c] / z);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (4 * j + c < F.act_dim) new_mean[m_at + 4 * j + c] = out[c];
}

template <bool PHYS>
void sampled_launch(const Params& P, const int L, const int NR, const float* phys, const PlanArgs& A, const PlanSampler& S, const float* mean,
                    float* returns, int32_t* steps, uint8_t* flags, float* last_obs, hipStream_t s) {
    const int grid = lane_grid(L, P.num_envs) * A.n_cand;   // (checked by the caller: fits the launch limit)
    with_task(P.task, [&](auto kind, auto task, auto nrs, auto fixed) {
        with_task_variant<task, nrs, fixed, 32>(L, NR, [&](auto l, auto nr) {   // (64 lanes per env: refused by the caller)
            rsx_launch((task_lookahead_sampled_kernel<kind, task, l, nr, PHYS>), dim3((unsigned)grid), dim3(64), 0, s, mean, returns, steps,
                       flags, last_obs, grid >> 3, P, A, S, phys);
        });
    });
}

PlanFlat flat_of(const Params& P, const uint32_t* ticks, const float* mean, const int n_candidates, const int horizon, const int act_dim) {
    return PlanFlat{mean, ticks, P.tick_base, P.env_id_base, P.num_envs, n_candidates, horizon, act_dim};
}

}  // namespace

void launch_task_lookahead_sampled(const Params& P, const int L, const int NR, const float* state, const float* aux, const uint32_t* ticks,
                                   const float* phys, const float* mean, const PlanSampler& S, const int n_candidates, const int horizon,
                                   const float gamma, float* returns, int32_t* steps, uint8_t* flags, float* last_obs, hipStream_t s) {
    const PlanArgs A{state, aux, ticks, n_candidates, horizon, gamma};
    if (phys) sampled_launch<true>(P, L, NR, phys, A, S, mean, returns, steps, flags, last_obs, s);
    else sampled_launch<false>(P, L, NR, nullptr, A, S, mean, returns, steps, flags, last_obs, s);
}

long long plan_flat_grid(const int num_envs, const int n_candidates, const int horizon, const int nblk) {
    const unsigned long long threads = (unsigned long long)num_envs * (unsigned long long)n_candidates * (unsigned long long)horizon * (unsigned long long)nblk;
    return (long long)((threads + 255ull) / 256ull);
}

void launch_plan_candidates(const Params& P, const uint32_t* ticks, const float* mean, const PlanSampler& S, const int n_candidates,
                            const int horizon, const int act_dim, float* out, hipStream_t s) {
    const long long grid = plan_flat_grid(P.num_envs, n_candidates, horizon, S.nblk);
    rsx_launch(plan_candidates_kernel, dim3((unsigned)grid), dim3(256), 0, s, out, flat_of(P, ticks, mean, n_candidates, horizon, act_dim), S);
}

void launch_plan_update(const Params& P, const uint32_t* ticks, const float* mean, const PlanSampler& S, const int n_candidates,
                        const int horizon, const int act_dim, const float* returns, const float temperature, float* new_mean, int32_t* best,
                        hipStream_t s) {
    const long long grid = plan_flat_grid(P.num_envs, 1, horizon, S.nblk);
    rsx_launch(plan_update_kernel, dim3((unsigned)grid), dim3(256), 0, s, returns, new_mean, best, temperature,
               flat_of(P, ticks, mean, n_candidates, horizon, act_dim), S);
}

}  // namespace rsx
