// rsx_plan.hip — exact lookahead over candidate action sequences (include/rsx.h: rsx_task_lookahead), in a translation unit of
// its own so that the instantiations of every existing kernel stay exactly what they were.
//
// task_lookahead_kernel runs, per (env, candidate) pair, up to `horizon` fused task steps from the env's CURRENT state with the
// candidate's actions in place of the fed action and the handle's real per-step draws (OU noise of the other robots) for the ticks
// the handle would take next, all in registers, and sums the discounted rewards.  It reads the handle's buffers and writes only
// its own outputs: the handle is left exactly as it was.
//
// The body is the `mode == 0` branch of rsx_task_step_body.inc built from the same device functions (load_raw, interpret_body,
// draw_for_step, physics, write_obs, task_reward) and the same three text fragments (rsx_step_commands.inc: actions -> commands,
// rsx_step_wire.inc, rsx_step_xr.inc: what the reward lane needs from the robots), the way
// trace_eval_phys_kernel (rsx_sysid.hip) was built from the raw step: between two steps the lane's record goes through the same
// wire-format round trip (heading in degrees, rate through deg/s, sin / cos re-derived from the stored heading, ball height through
// r_ball + z) that a store and a reload apply, so a pair's rewards, flags and observations are bit for bit those of `horizon`
// rsx_task_step calls with the candidate's actions.  What the step body does at an episode end — placement, auto-reset, physics
// redraw, metrics — is NOT simulated: a pair stops at its env's first episode end.
//
// Grid: one lane group per pair, tiles(num_envs) x K workgroups.  Workgroup -> (tile, candidate): the XCD's share of the grid is
// cut into runs of K consecutive workgroups that hold the K candidates of ONE tile, so the state rows of a tile are fetched from
// HBM once per XCD and the other K - 1 groups find them in that XCD's L2.
//
// The loop itself is rsx_plan_body.inc, shared with the kernel that draws its candidates instead of loading them
// (rsx_plan_sampled.hip); this unit supplies the loads.
//
// Registers: the per-pair accumulators (return, discount, step count, flags) are plain scalars held by every lane and advanced
// through selects — indexed by role they would go to scratch memory (see the note on Acc in rsx_sysid.hip).  The observation is
// written once per pair (at its end or after the last step), not per step.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rsx.h"
#include "rsx_plan_common.hpp"
#include "rsx_units.hpp"
#include "rsx_variants.hpp"

namespace rsx {

namespace {

template <int KIND, int TASK, int L, int NR, bool PHYS>
__global__ __launch_bounds__(64) void task_lookahead_kernel(const float* __restrict__ actions, float* __restrict__ returns,
                                                            int32_t* __restrict__ steps_out, uint8_t* __restrict__ flags_out,
                                                            float* __restrict__ last_obs, const int per_xcd, const Params P,
                                                            const PlanArgs A, const float* __restrict__ phys) {
// where a step's action comes from: the caller's tensor [num_envs][K][H][act_dim]
#define RSX_PLAN_ACT_SETUP \
    const float* const my_act = actions + pair * (size_t)A.horizon * step_floats + (TASK == RSX_TASK_SSL_SCRIMMAGE ? (size_t)b * AD : 0);
#define RSX_PLAN_ACT_FETCH(DST, STEP) \
    _Pragma("unroll") for (int i = 0; i < AD; ++i) DST[i] = my_act[(size_t)(STEP) * step_floats + i];
#include "rsx_plan_body.inc"
#undef RSX_PLAN_ACT_SETUP
#undef RSX_PLAN_ACT_FETCH
}

template <bool PHYS>
void plan_launch(const Params& P, const int L, const int NR, const float* phys, const PlanArgs& A, const float* actions, float* returns,
                 int32_t* steps, uint8_t* flags, float* last_obs, hipStream_t s) {
    const int grid = lane_grid(L, P.num_envs) * A.n_cand;   // (checked by the caller: fits the launch limit)
    with_task(P.task, [&](auto kind, auto task, auto nrs, auto fixed) {
        with_task_variant<task, nrs, fixed, 32>(L, NR, [&](auto l, auto nr) {   // (64 lanes per env: refused by rsx_task_lookahead)
            rsx_launch((task_lookahead_kernel<kind, task, l, nr, PHYS>), dim3((unsigned)grid), dim3(64), 0, s, actions, returns, steps, flags,
                       last_obs, grid >> 3, P, A, phys);
        });
    });
}

}  // namespace

long long lookahead_grid(const int L, const int num_envs, const int n_candidates) {
    return (long long)lane_grid(L, num_envs) * (long long)n_candidates;
}

void launch_task_lookahead(const Params& P, const int L, const int NR, const float* state, const float* aux, const uint32_t* ticks,
                           const float* phys, const float* actions, const int n_candidates, const int horizon, const float gamma,
                           float* returns, int32_t* steps, uint8_t* flags, float* last_obs, hipStream_t s) {
    const PlanArgs A{state, aux, ticks, n_candidates, horizon, gamma};
    if (phys) plan_launch<true>(P, L, NR, phys, A, actions, returns, steps, flags, last_obs, s);
    else plan_launch<false>(P, L, NR, nullptr, A, actions, returns, steps, flags, last_obs, s);
}

}  // namespace rsx
