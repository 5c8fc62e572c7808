// rsx_layout.hpp — which kernel layout steps a handle's envs: the thresholds and the one function that applies them.
//
// Every layout gives identical results; the choice is one of speed.  rsx_task_attach and rsx_physics_enable call
// plan_layout, the handle keeps the StepPlan, and the dispatch, the tick-slot grid, rsx_task_rollout and rsx_task_layout read it
// (rsx_api_task.hip).  No HIP include: tests/test_layout_plan.py compiles this header with the host compiler alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>

#include "rsx.h"
#include "rsx_params.hpp"

// smallest batch stepped by the one-lane-per-env kernels: measured crossovers of single-step launches (round 3,
// gpurun_out/xover.txt -> profiles/r03_layout_crossovers.txt; multi-step launches cross earlier): VSS-v0 98 304 envs
// (31.5 vs 29.3 us), static defenders 65 536 (29.2 vs 28.5), dribbling 49 152 (30.0 vs 29.2), contested possession
// 32 768 (19.5 vs 18.8), pass endurance 32 768 (17.8 vs 15.3)
#ifndef RSX_EPL_MIN_ENVS
#define RSX_EPL_MIN_ENVS 98304
#endif
#ifndef RSX_EPL_MIN_ENVS_SSL
#define RSX_EPL_MIN_ENVS_SSL 65536
#endif
constexpr int RSX_EPL_MIN_ENVS_DRIBBLING = 49152, RSX_EPL_MIN_ENVS_DUEL = 32768;   // (DUEL: contested possession, pass endurance)
// smallest batch of the SSL 11v11 scrimmage task stepped by the large-batch build of its kernel (rsx_big.hip)
#ifndef RSX_BIG_MIN_ENVS
#define RSX_BIG_MIN_ENVS 8192
#endif
// smallest batches of the scrimmage task stepped by the four-lanes-per-env kernel (RSX_LAYOUT=quad|lanes overrides).  Measured
// crossovers (profiles/LABBOOK.md): the spread line-up from 32 768 envs, the crowded one (contacts in every sub-step: the six
// robots of a lane are walked one after the other) from 65 536
#ifndef RSX_QUAD_MIN_ENVS
#define RSX_QUAD_MIN_ENVS 32768
#endif
#ifndef RSX_QUAD_MIN_ENVS_CROWDED
#define RSX_QUAD_MIN_ENVS_CROWDED 65536
#endif
// from this batch on a multi-step call (rsx_task_rollout) on a four-lane handle is issued as single-step launches: n launches of
// the four-lanes-per-env kernel beat one launch of the 32-lane kernel (262 144 envs, us per step: spread 182 vs 275, crowded 298
// vs 340; crowded 131 072: 161 vs 164); same steps, same results
#ifndef RSX_QUAD_ROLLOUT_MIN_ENVS
#define RSX_QUAD_ROLLOUT_MIN_ENVS 49152
#endif
#ifndef RSX_QUAD_ROLLOUT_MIN_ENVS_CROWDED
#define RSX_QUAD_ROLLOUT_MIN_ENVS_CROWDED 196608
#endif
// largest batch of VSS-v0 3v3 whose single steps run in the paired form (rsx_pair.hpp: a service wave next to each physics wave;
// RSX_SERVICE_WAVE=0|1 overrides).  Measured, one build, RSX_SERVICE_WAVE=0 vs 1, us per step (profiles/LABBOOK.md, "A service wave
// for the VSS-v0 3v3 single step"): 2048 envs 8.77 vs 8.31 (-5.3 %), 4096 envs 9.45 vs 9.17 (-3.0 %), 6144 envs 9.73 vs 9.55 (-1.9 %),
// 8192 envs 9.91 vs 9.81 (-1.0 %).  The form still wins above 4096 envs, where the service waves no longer find SIMDs of their own
// (2 x tiles > 1024 on this part), but by less than the 2 % that keeps a change: the threshold is the last measured batch that clears it.
#ifndef RSX_SERVICE_WAVE_MAX_ENVS
#define RSX_SERVICE_WAVE_MAX_ENVS 4096
#endif

namespace rsx {

// Lanes: the lane-group kernels (8 / 16 / 32 / 64 lanes per env); LanesBig: the large-batch build of the 32-lane scrimmage kernel;
// Quad: four lanes per env (scrimmage, single steps only); Epl: one lane per env
enum class Layout { Lanes, LanesBig, Quad, Epl };

struct StepPlan {
    Layout step = Layout::Lanes;      // single-step launches (MODE_STEP)
    Layout rollout = Layout::Lanes;   // one-launch rollouts (MODE_ROLLOUT); resets always run on the lane-group kernels
    bool rollout_as_steps = false;    // rsx_task_rollout issues n single-step launches instead of one launch
    bool service_wave = false;        // single-step launches of Layout::Lanes run the paired form (VSS-v0 3v3 only; rollouts and resets never)
};

struct LayoutQuery {
    int task, kind, L, NR, n_blue, num_envs, row_stride, state_dim, obs_dim, n_sub;
    bool physics;             // per-env physics is on (rsx_physics_enable)
    const char* env_layout;   // the value of RSX_LAYOUT, or null (the caller reads the environment)
    const char* env_service;  // the value of RSX_SERVICE_WAVE ("0" / "1"), or null
};

inline StepPlan plan_layout(const LayoutQuery& q) {
    StepPlan p;
    if (q.physics) return p;   // per-env physics: the lane-group kernels at every batch size
    const auto asked = [&](const char* name) { return q.env_layout && std::strcmp(q.env_layout, name) == 0; };
    // the one- and four-lane kernels address rows with 32-bit byte offsets: arrays of 2 GB and more stay with the lane-group kernels
    const int task = q.task, n_robots = (q.state_dim - 5) / (q.kind == RSX_KIND_VSS ? ModelD<RSX_KIND_VSS>::rs : ModelD<RSX_KIND_SSL>::rs);
    const size_t rows = (size_t)std::max(q.state_dim + X_ROWS, aux_rows(n_robots));
    const bool rows_below_2g = rows * (size_t)q.row_stride * sizeof(float) < ((size_t)1 << 31);
    if ((task == RSX_TASK_SSL_SCRIMMAGE || task == RSX_TASK_SSL_SCRIMMAGE_CROWDED) && q.NR == 22 && q.L == 32) {
        const bool spread = task == RSX_TASK_SSL_SCRIMMAGE;
        p.step = p.rollout = q.num_envs >= RSX_BIG_MIN_ENVS ? Layout::LanesBig : Layout::Lanes;
        // four lanes per env: a real time step (the infrared row is rewritten), 11 blue robots.  RSX_LAYOUT=lanes: off, the large-batch build stays
        const int quad_min = spread ? RSX_QUAD_MIN_ENVS : RSX_QUAD_MIN_ENVS_CROWDED;
        const bool fits = rows_below_2g && q.n_sub > 0 && q.n_blue == 11;
        if (fits && (q.env_layout ? asked("quad") : (quad_min > 0 && q.num_envs >= quad_min))) {
            p.step = Layout::Quad;
            p.rollout_as_steps = q.num_envs >= (spread ? RSX_QUAD_ROLLOUT_MIN_ENVS : RSX_QUAD_ROLLOUT_MIN_ENVS_CROWDED);
        }
        return p;
    }
    // The five registered tasks: the one-lane-per-env kernel needs enough envs to fill the chip with its long waves
    const bool fixed_ssl = task == RSX_TASK_SSL_DRIBBLING || task == RSX_TASK_SSL_CONTESTED || task == RSX_TASK_SSL_PASS_ENDURANCE;   // team sizes checked by derive_task
    if ((task == RSX_TASK_VSS_V0 && q.NR == 6 && q.L == 8) || (task == RSX_TASK_SSL_STATIC_DEFENDERS && q.NR == 7 && q.L == 8) || fixed_ssl) {
        const int epl_min = task == RSX_TASK_VSS_V0 ? RSX_EPL_MIN_ENVS : task == RSX_TASK_SSL_STATIC_DEFENDERS ? RSX_EPL_MIN_ENVS_SSL
                          : task == RSX_TASK_SSL_DRIBBLING ? RSX_EPL_MIN_ENVS_DRIBBLING : RSX_EPL_MIN_ENVS_DUEL;
        const bool epl = asked("epl") || (!asked("lanes") && q.num_envs >= epl_min);
        if (epl && rows_below_2g && (size_t)q.num_envs * q.obs_dim * sizeof(float) < ((size_t)1 << 31)) p.step = p.rollout = Layout::Epl;
    }
    // the paired single step: the one variant that is built (8 lanes per env, kernels specialised for 3v3), where the lane-group kernels step
    if (task == RSX_TASK_VSS_V0 && q.NR == 6 && q.L == 8 && p.step == Layout::Lanes)
        p.service_wave = q.env_service ? std::strcmp(q.env_service, "1") == 0 : q.num_envs <= RSX_SERVICE_WAVE_MAX_ENVS;
    return p;
}

}  // namespace rsx
