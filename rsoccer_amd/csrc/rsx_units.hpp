// rsx_units.hpp — what one translation unit of librsx_hip.so defines and another calls.  The defining unit includes this header
// too, so a signature that drifts is a compile error in that unit, not an undefined symbol when the library is loaded.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rsx {

struct Params;
struct Buffers;

// rsx_epl.hip: the one-lane-per-env kernels (large batches) and the four-lanes-per-env kernel of the SSL 11v11 scrimmage task
// (single-step launches, n_steps = 1 | flags); *_grid: workgroups of those launches (the host sizes the per-workgroup tick slots
// from these: rsx_kernels.hpp, step_tick)
void launch_vss_epl(bool rollout, const Params& P, const Buffers& b, int n_steps, hipStream_t s);
void launch_ssl_epl(int task, bool rollout, const Params& P, const Buffers& b, int n_steps, hipStream_t s);
void launch_ssl_quad(const Params& P, const Buffers& b, int n_steps, hipStream_t s);
int epl_grid(int num_envs);
int ssl_quad_grid(int num_envs);
// rsx_big.hip: the 32-lanes-per-env kernel of the scrimmage task built for large batches
void launch_scrimmage_big(bool rollout, const Params& P, const Buffers& b, int n_steps, hipStream_t s);
// rsx_phys.hip: the kernels of physics-enabled handles (rsx_physics_enable)
void launch_task_phys(const Params& P, const Buffers& b, int L, int NR, float* phys, int n_steps, int mode, hipStream_t s);
void launch_sim_phys(const Params& P, const Buffers& b, int L, int NR, float* phys, float* state_out, int rand_tick, hipStream_t s);
void launch_phys_init(float* blk, int B, int S, int kind, int ts_ms, hipStream_t s);
void launch_phys_set(float* blk, const float* vals, const uint8_t* mask, int B, int S, int vstride, hipStream_t s);
void launch_phys_ranges(float* blk, const float* lo, const float* hi, uint32_t mask, hipStream_t s);
// rsx_sysid.hip: trace evaluation (rsx_trace_eval)
void launch_trace_eval(const Params& P, int L, int NR, const float* phys, float* state, float* loss, const float* frames,
                       const float* cmds, const int32_t* anchors, int n_frames, int n_anchors, int horizon, hipStream_t s);

}  // namespace rsx
