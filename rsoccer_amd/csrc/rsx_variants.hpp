// rsx_variants.hpp — which compiled kernel variant serves a handle, and how its launch is shaped: host side, written down once
// for every translation unit of librsx_hip.so.
//
// A handle carries two run-time numbers, L (lanes per env) and NR (the robot count its kernels were specialised for, 0 = the
// generic build).  The selectors below turn them — and the mode and task id of a call — into compile-time constants and hand
// them to a functor as std::integral_constant values; the functor names the unit's own kernel template:
//
//     with_sim_variant<KIND, 64>(L, NR, [&](auto l, auto nr) { launch_sim_hot(sim_step_kernel<KIND, l, nr>, ...); });
//
// The SET of instantiations is the selectors' to decide and differs per unit only by MAX_L: the literal kernels exist for 64
// lanes per env, the per-env physics and trace kernels do not (rsx_physics_enable refuses such handles).  The (COND ? N : 0)
// guards keep a branch that can never be taken for this KIND / TASK from instantiating a kernel of its own.
//
// Not here: the choice of LAYOUT for a handle (one lane per env, four lanes per env, the large-batch build, placement helpers,
// the per-env physics route, the paired single step of VSS-v0 3v3 — one variant, named by rsx_pair.hip itself) — rsx_layout.hpp decides that (plan_layout), and rsx_api_task.hip dispatches on it in front of these tables.
#pragma once
#include <type_traits>
#include <utility>

#include "rsx_launch.hpp"
#include "rsx_kernels.hpp"

namespace rsx {

template <int V> using int_c = std::integral_constant<int, V>;

// (grids of a launch and the variant policy, specialised_robots: rsx_params.hpp — the host units need them without the kernels)

// the generic variant of a lane-group width
template <int MAX_L, typename F>
void with_generic_variant(const int L, F&& f) {
    static_assert(MAX_L == 32 || MAX_L == 64, "widest lane group the unit instantiates");
    switch (L) {
        case 8: f(int_c<8>{}, int_c<0>{}); break;
        case 16: f(int_c<16>{}, int_c<0>{}); break;
        case 32: f(int_c<32>{}, int_c<0>{}); break;
        default: f(int_c<MAX_L>{}, int_c<0>{}); break;
    }
}

// raw step (and what is built like it: trace evaluation): f(l, nr)
template <int KIND, int MAX_L, typename F>
void with_sim_variant(const int L, const int NR, F&& f) {
    if (KIND == RSX_KIND_VSS && NR == 6 && L == 8) { f(int_c<8>{}, int_c<(KIND == RSX_KIND_VSS ? 6 : 0)>{}); return; }
    if (KIND == RSX_KIND_VSS && NR == 10) { f(int_c<16>{}, int_c<(KIND == RSX_KIND_VSS ? 10 : 0)>{}); return; }
    if (KIND == RSX_KIND_SSL && NR == 7 && L == 8) { f(int_c<8>{}, int_c<(KIND == RSX_KIND_SSL ? 7 : 0)>{}); return; }
    if (KIND == RSX_KIND_SSL && NR == 12) { f(int_c<16>{}, int_c<(KIND == RSX_KIND_SSL ? 12 : 0)>{}); return; }
    if (KIND == RSX_KIND_SSL && NR == 22) { f(int_c<32>{}, int_c<(KIND == RSX_KIND_SSL ? 22 : 0)>{}); return; }
    with_generic_variant<MAX_L>(L, f);
}

// task step of a task registered with NRS robots: f(l, nr).  FIXED: the task fixes its team sizes — one variant, 8 lanes per
// env, exact robot count
template <int TASK, int NRS, bool FIXED, int MAX_L, typename F>
void with_task_variant(const int L, const int NR, F&& f) {
    if constexpr (FIXED) {
        f(int_c<8>{}, int_c<NRS>{});
    } else {
        if (NRS <= 7 && NR == NRS && L == 8) { f(int_c<8>{}, int_c<(NRS <= 7 ? NRS : 0)>{}); return; }
        if (NRS <= 7 && NR == NRS && L == 16) { f(int_c<16>{}, int_c<(NRS <= 7 ? NRS : 0)>{}); return; }
        if (TASK == RSX_TASK_SSL_SCRIMMAGE && NR == 22 && L == 32) { f(int_c<32>{}, int_c<(TASK == RSX_TASK_SSL_SCRIMMAGE ? 22 : 0)>{}); return; }   // 11v11
        if (TASK == RSX_TASK_VSS_V0 && NR == 10 && L == 16) { f(int_c<16>{}, int_c<(TASK == RSX_TASK_VSS_V0 ? 10 : 0)>{}); return; }   // VSS-v0 on the 5v5 field
        with_generic_variant<MAX_L>(L, f);
    }
}

// task id -> f(kind, task, nrs, fixed): the task's kernels (the crowded scrimmage shares the scrimmage's)
template <typename F>
void with_task(const int task, F&& f) {
    switch (task) {
        case RSX_TASK_VSS_V0: f(int_c<RSX_KIND_VSS>{}, int_c<RSX_TASK_VSS_V0>{}, int_c<6>{}, std::false_type{}); break;
        case RSX_TASK_SSL_STATIC_DEFENDERS: f(int_c<RSX_KIND_SSL>{}, int_c<RSX_TASK_SSL_STATIC_DEFENDERS>{}, int_c<7>{}, std::false_type{}); break;
        case RSX_TASK_SSL_DRIBBLING: f(int_c<RSX_KIND_SSL>{}, int_c<RSX_TASK_SSL_DRIBBLING>{}, int_c<5>{}, std::true_type{}); break;
        case RSX_TASK_SSL_CONTESTED: f(int_c<RSX_KIND_SSL>{}, int_c<RSX_TASK_SSL_CONTESTED>{}, int_c<2>{}, std::true_type{}); break;
        case RSX_TASK_SSL_SCRIMMAGE: case RSX_TASK_SSL_SCRIMMAGE_CROWDED:
            f(int_c<RSX_KIND_SSL>{}, int_c<RSX_TASK_SSL_SCRIMMAGE>{}, int_c<22>{}, std::false_type{}); break;
        default: f(int_c<RSX_KIND_SSL>{}, int_c<RSX_TASK_SSL_PASS_ENDURANCE>{}, int_c<2>{}, std::true_type{}); break;
    }
}

// mode: MODE_STEP (one step, optional fed actions; n_steps = 1 | flags), MODE_ROLLOUT (n_steps in one launch), MODE_RESET,
// MODE_REFRESH -> f(mode)
template <typename F>
void with_mode(const int mode, F&& f) {
    switch (mode) {
        case MODE_STEP: f(int_c<MODE_STEP>{}); break;
        case MODE_ROLLOUT: f(int_c<MODE_ROLLOUT>{}); break;
        case MODE_RESET: f(int_c<MODE_RESET>{}); break;
        default: f(int_c<MODE_REFRESH>{}); break;
    }
}
// ... and what a launch of that mode is given: only the stepping modes a step count
inline int mode_steps(const int mode, const int n_steps) { return mode == MODE_STEP || mode == MODE_ROLLOUT ? n_steps : 1; }

// ---- launches ----------------------------------------------------------------------------------------------------------
// Workgroups of a launch of a kernel with the RSX_HOT_ARGS parameter list: `tiles` of them map to tiles, `helpers` more sit
// behind them (the tile map still sees the tile grid); `lds`: dynamic LDS; `per_xcd`: the tile-map argument where it is not
// tiles / 8 (the zig-zag order of the one-lane-per-env single steps), 0 = tiles / 8; `threads`: per workgroup — one wave, or the two of
// the paired single step (rsx_pair.hpp)
struct HotGrid {
    int tiles, helpers = 0;
    size_t lds = 0;
    int per_xcd = 0;
    int threads = 64;
};

// hot arguments first (preloaded into SGPRs, see RSX_HOT_ARGS), then the by-value structs, then the unit's own trailing
// arguments.  `out` / `in`: the second and third pointer slot
template <typename... KArgs, typename... Tail>
void launch_hot(void (*kernel)(KArgs...), const HotGrid& g, hipStream_t s, float* out, const float* in, const int n, const Params& P,
                const Buffers& b, Tail&&... tail) {
    rsx_launch(kernel, dim3((unsigned)(g.tiles + g.helpers)), dim3((unsigned)g.threads), g.lds, s, b.state, out, in, b.flags, P.num_envs,
               RSX_HOT_DIM(P.state_dim, P.row_stride, P.num_envs), g.per_xcd ? g.per_xcd : g.tiles >> 3, n, P, b, std::forward<Tail>(tail)...);
}
// task step: aux rows and fed actions, n_steps
template <typename... KArgs, typename... Tail>
void launch_task_hot(void (*kernel)(KArgs...), const HotGrid& g, hipStream_t s, const int n_steps, const Params& P, const Buffers& b, Tail&&... tail) {
    launch_hot(kernel, g, s, b.aux, b.actions, n_steps, P, b, std::forward<Tail>(tail)...);
}
// raw step: where the new state goes and the commands, rand_tick
template <typename... KArgs, typename... Tail>
void launch_sim_hot(void (*kernel)(KArgs...), const HotGrid& g, hipStream_t s, float* state_out, const int rand_tick, const Params& P, const Buffers& b, Tail&&... tail) {
    launch_hot(kernel, g, s, state_out, b.cmds, rand_tick, P, b, std::forward<Tail>(tail)...);
}

}  // namespace rsx
