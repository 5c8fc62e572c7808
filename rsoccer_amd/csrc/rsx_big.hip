// rsx_big.hip — the lane-group kernels once more, compiled for LARGE batches (own translation unit, own flags).
//
// rsx_lanes.hip builds task_step_kernel with -amdgpu-sched-strategy=max-ilp: at the benchmark batches a SIMD holds one
// wave and latency has to be hidden inside it.  From a few thousand waves on the opposite holds — registers, i.e.
// waves per SIMD, are what hides latency — so the configurations that have no one-lane-per-env kernel (SSL 11v11:
// 32 lanes per env) are built here a second time with the default scheduler and without the SLP vectorizer, under
// another symbol name, and the host picks by batch size (rsx_layout.hpp: RSX_BIG_MIN_ENVS).  Same source, same results.
#include <hip/hip_runtime.h>

#define task_step_kernel task_step_kernel_big
#include "rsx_kernels.hpp"

#include "rsx_units.hpp"
#include "rsx_variants.hpp"

namespace rsx {

void launch_scrimmage_big(bool rollout, const Params& P, const Buffers& b, int n_steps, hipStream_t s) {
    const HotGrid grid{lane_grid(32, P.num_envs)};
    if (rollout) launch_task_hot((task_step_kernel_big<RSX_KIND_SSL, 32, RSX_TASK_SSL_SCRIMMAGE, 22, MODE_ROLLOUT>), grid, s, n_steps, P, b);
    else launch_task_hot((task_step_kernel_big<RSX_KIND_SSL, 32, RSX_TASK_SSL_SCRIMMAGE, 22, MODE_STEP>), grid, s, n_steps, P, b);
}

}  // namespace rsx
