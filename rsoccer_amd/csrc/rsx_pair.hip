// rsx_pair.hip — the paired form of the fused VSS-v0 single step (rsx_pair.hpp: task_pair_step_kernel, workgroups of a physics wave and
// a service wave), in a translation unit of its own: the instantiations of rsx_lanes.hip stay as they were.  Scheduler as for rsx_lanes.hip.
#include <hip/hip_runtime.h>

#include "rsx.h"
#include "rsx_units.hpp"
#include "rsx_variants.hpp"
#include "rsx_pair.hpp"

namespace rsx {

// the grid of launch_task for the same handle (one workgroup per tile, no helpers), 128 threads per workgroup: the tick slots of a
// device-keyed handle are the same ones whichever form steps it
void launch_task_pair(const Params& P, const Buffers& b, int n_steps, hipStream_t s) {
    HotGrid g{lane_grid(8, P.num_envs)};
    g.threads = 128;
    launch_task_hot((task_pair_step_kernel<RSX_KIND_VSS, 8, RSX_TASK_VSS_V0, 6, MODE_STEP>), g, s, n_steps, P, b);
}

}  // namespace rsx
