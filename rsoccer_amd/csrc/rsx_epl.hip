// rsx_epl.hip — the one-lane-per-env kernels (VSS-v0 and the four SSL tasks) in their own translation unit:
// built with the compiler's default machine scheduler and explicit occupancy targets per entry point, while
// rsx_lanes.hip is built with -amdgpu-sched-strategy=max-ilp, which suits the short 8-lanes-per-env kernels at
// small batches but costs these a wave of occupancy.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "rsx_epl.hpp"
#include "rsx_epl_ssl.hpp"
#include "rsx_quad_ssl.hpp"
#include "rsx_units.hpp"
#include "rsx_variants.hpp"

namespace rsx {

// development knob: RSX_EPL_LDS_PAD=<bytes> of dynamic LDS per workgroup limit the waves per CU (occupancy
// sensitivity measurements); 0 in production
// tile order of a single-step launch: alternates with the step counter (tile_of_block_zigzag, rsx_hot_args.hpp);
// RSX_EPL_ZIGZAG=0 keeps one direction (development A/B)
// (device-keyed launches — n_steps carries RSX_TICK_DEV — cannot be told the parity: a negative `per` asks the kernel to alternate)
static int step_per_xcd(const Params& P, const int grid, const int n_steps) {
    static const bool zig = !(std::getenv("RSX_EPL_ZIGZAG") && std::atoi(std::getenv("RSX_EPL_ZIGZAG")) == 0);
    const int per = grid >> 3;
    if (n_steps & RSX_TICK_DEV) return zig ? -per : per;
    return (zig && (P.tick_base & 1u)) ? -per : per;
}

#ifndef RSX_SD_LEAN_MAX_ENVS
#define RSX_SD_LEAN_MAX_ENVS 786432
#endif

static unsigned epl_lds_pad() {
    static const unsigned pad = std::getenv("RSX_EPL_LDS_PAD") ? (unsigned)std::atoi(std::getenv("RSX_EPL_LDS_PAD")) : 0u;
    return pad;
}

void launch_vss_epl(bool rollout, const Params& P, const Buffers& b, int n_steps, hipStream_t s) {
    const int grid = epl_grid(P.num_envs);
    if (rollout) launch_task_hot(vss_epl_rollout_kernel, {grid}, s, n_steps, P, b);
    else launch_task_hot((vss_epl_kernel<MODE_STEP>), {grid, 0, epl_lds_pad(), step_per_xcd(P, grid, n_steps)}, s, n_steps, P, b);
}

template <int TASK>
static void launch_ssl_epl_t(bool rollout, const Params& P, const Buffers& b, int n_steps, hipStream_t s) {
    const int grid = epl_grid(P.num_envs);
    if (rollout) { launch_task_hot((ssl_epl_kernel<TASK, MODE_ROLLOUT>), {grid}, s, n_steps, P, b); return; }
    // the lean single-step form (rsx_epl_ssl.hpp): 1v6 below RSX_SD_LEAN_MAX_ENVS (occupancy-bound there: 262 144 envs 52 -> 47 us;
    // at 1 M envs, bandwidth-bound, the classic form is 4-7 % faster), contested possession always (-5 %); measured equal
    // or worse for dribbling and pass endurance (episodes of a few steps: most waves store the robot rows twice)
    const char* const fe = std::getenv("RSX_EPL_LEAN");   // 0 / 1: tests and A/B runs (read per launch: tests switch it inside one process)
    const int force = fe ? std::atoi(fe) : -1;
    const bool lean = force >= 0 ? force != 0
                                 : TASK == RSX_TASK_SSL_CONTESTED || (TASK == RSX_TASK_SSL_STATIC_DEFENDERS && P.num_envs < RSX_SD_LEAN_MAX_ENVS);
    const HotGrid g{grid, 0, 0, step_per_xcd(P, grid, n_steps)};
    if (lean && (TASK == RSX_TASK_SSL_CONTESTED || TASK == RSX_TASK_SSL_STATIC_DEFENDERS))
        launch_task_hot((ssl_epl_kernel<TASK, MODE_STEP, (TASK == RSX_TASK_SSL_CONTESTED || TASK == RSX_TASK_SSL_STATIC_DEFENDERS)>), g, s, n_steps, P, b);
    else
        launch_task_hot((ssl_epl_kernel<TASK, MODE_STEP>), g, s, n_steps, P, b);
}

void launch_ssl_quad(const Params& P, const Buffers& b, int n_steps, hipStream_t s) {   // SSL 11v11 scrimmage, four lanes per env, single-step launches (n_steps = 1 | flags)
    const int grid = ssl_quad_grid(P.num_envs);
    launch_task_hot((ssl_quad_kernel<MODE_STEP>), {grid, 0, 0, step_per_xcd(P, grid, n_steps)}, s, n_steps, P, b);
}

// workgroups of a launch
int ssl_quad_grid(int num_envs) { return tile_grid((num_envs + Q_ENVS - 1) / Q_ENVS); }
int epl_grid(int num_envs) { return env_grid(num_envs); }

void launch_ssl_epl(int task, bool rollout, const Params& P, const Buffers& b, int n_steps, hipStream_t s) {
    switch (task) {
        case RSX_TASK_SSL_STATIC_DEFENDERS: launch_ssl_epl_t<RSX_TASK_SSL_STATIC_DEFENDERS>(rollout, P, b, n_steps, s); break;
        case RSX_TASK_SSL_DRIBBLING: launch_ssl_epl_t<RSX_TASK_SSL_DRIBBLING>(rollout, P, b, n_steps, s); break;
        case RSX_TASK_SSL_CONTESTED: launch_ssl_epl_t<RSX_TASK_SSL_CONTESTED>(rollout, P, b, n_steps, s); break;
        default: launch_ssl_epl_t<RSX_TASK_SSL_PASS_ENDURANCE>(rollout, P, b, n_steps, s); break;
    }
}

}  // namespace rsx

#ifdef RSX_QSTATS
extern "C" __attribute__((visibility("default"))) int rsx_debug_qstats(unsigned long long* out, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(rsx::rsx_qstats), sizeof(unsigned long long) * 16) != hipSuccess) return -1;
    if (reset) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(rsx::rsx_qstats), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
#endif
