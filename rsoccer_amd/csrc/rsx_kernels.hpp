// rsx_kernels.hpp — the per-env.step() hot path as hand-written HIP for gfx950 (CDNA4).
//
// Replaces robosim.VSS.step / robosim.SSL.step (+ get_state) — reference call sites
// rsoccer_gym/Simulators/rsim.py:102,105,155,158 — and, in the fused task variants, the Python
// hooks around them: VSSEnv._get_commands/_frame_to_observations/_calculate_reward_and_done
// (vss/env_vss/vss_gym.py:93-192) and the same three of SSLHWStaticDefendersEnv
// (ssl/ssl_hw_challenge/static_defenders.py:90-212), TimeLimit and reset placement.
//
// Mapping (wave64):
//   * one lane owns one rigid body (robot or ball); an env occupies a group of L lanes
//     (L = 8 for <= 7 robots, 16, 32, or 64 = the whole wavefront) and a wave hosts G = 64/L
//     envs.  L >= 16: lane = body * G + env_in_wave, so the G lanes that own "body k" of
//     neighbouring envs are adjacent and read adjacent floats of SoA row k (G*4 contiguous bytes
//     per body).  L = 8: lane = env_in_wave * 8 + body (LaneMap, rsx_lane_map.hpp; measured -1 % at the
//     latency-bound batches, +2-3 % at 65 536 envs).  Either way a wave touches the same 32-byte
//     pieces, and the 6..11 rows of one body share cache lines with the neighbouring tiles handled
//     by the SAME XCD (tile -> XCD map: rsx_hot_args.hpp), so every byte fetched into an L2 is used.
//   * the all-pairs contact test is a Jacobi sweep: each lane publishes (x, y, vx, vy) as one
//     float4 in LDS and reads the other bodies' float4 back (ds_read_b128, broadcast inside a
//     group, G distinct 16-B slots per instruction -> conflict free).  With the robot count a
//     template constant the sweep is fully unrolled, so all reads of a sub-step are in flight
//     together and their latency is paid once.  All sub-steps of one env.step() run out of
//     registers + LDS; HBM is touched once for the load and once for the store of the state.
//   * SSL: the robot lane evaluates its own robot-ball contact (kicker-mouth geometry) and
//     publishes the ball-side impulse / dribbler / kick record; the ball lane learns from one
//     ballot which robots wrote one and sums those in index order.  No lane re-derives another
//     lane's geometry.
//   * a single-step launch lasts as long as its slowest wave, so the rare paths are shaped for
//     the wave that takes them: the overlap test of a sweep is one integer minimum and one
//     compare, each lane then walks only ITS partners (lanes with different partners share an
//     iteration), and the reset placement of an ended env is done by all of its lanes together
//     (place_env_parallel).
//   * 64-thread workgroups (one wave): a 4096-env VSS batch is 512 workgroups, two per CU,
//     so all 256 CUs work; block b runs on XCD b % 8 and is mapped to tile
//     (b % 8) * tiles_per_xcd + b / 8 so each XCD's L2 sees one contiguous 1/8 of every row.
//   * fp32 throughout, -ffp-contract=off, fixed summation order (body index order) -> results
//     are bit-identical for any batch size, position in the batch, L, or shard.
//   * scalar registers: class/task constants are instruction literals (KC<>, TC<>); only the
//     run-time block `Params` and 8 base pointers live in SGPRs.
//
// This file holds the four kernel templates and nothing else; what they are made of, in the order it builds up:
//   rsx_lane_map.hpp   lane <-> (body, env), the LDS record, addressing                 (needs nothing of the simulator)
//   rsx_hot_args.hpp   tile map, preloaded kernel arguments, metrics line, step counter  (rsx_params.hpp)
//   rsx_state_io.hpp   load / interpret / store of a body in wire format                 (rsx_body.hpp, rsx_lane_map.hpp)
//   rsx_contact.hpp    physics(): sub-steps and contact sweeps, per-env coefficients     (rsx_body.hpp, rsx_phys.hpp, rsx_lane_map.hpp)
//   rsx_task.hpp       observations, commands, reward, per-step draws                    (rsx_math.hpp, rsx_params.hpp)
//   rsx_placement.hpp  reset placement and its cache                                     (rsx_lane_map.hpp)
// and the kernel bodies, included as text: rsx_sim_step_body.inc, rsx_task_step_body.inc (which shares rsx_step_commands.inc,
// rsx_step_wire.inc and rsx_step_xr.inc with the lookahead's rsx_plan_body.inc).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "rsx_math.hpp"
#include "rsx_params.hpp"
#include "rsx_body.hpp"
#include "rsx_phys.hpp"
#include "rsx_lane_map.hpp"
#include "rsx_hot_args.hpp"
#include "rsx_state_io.hpp"
#include "rsx_contact.hpp"
#include "rsx_task.hpp"
#include "rsx_placement.hpp"

namespace rsx {

// =============================================================================================
// raw simulator step: robosim.step(cmds) + get_state() on the SoA buffers
// =============================================================================================
template <int KIND, int L, int NR>
__global__ __launch_bounds__(64) void sim_step_kernel(RSX_HOT_ARGS, const Params P_, const Buffers bufs_) {
    constexpr bool PHYS = false;
    const float* const phys = nullptr;
#include "rsx_sim_step_body.inc"
}
// the raw step of a physics-enabled handle (rsx_physics_enable): the same, each env with its own coefficients
// (rsx_phys.hpp: EnvCoef from the coefficient rows of the block `phys`)
template <int KIND, int L, int NR>
__global__ __launch_bounds__(64) void sim_step_phys_kernel(RSX_HOT_ARGS, const Params P_, const Buffers bufs_, const float* phys) {
    constexpr bool PHYS = true;
#include "rsx_sim_step_body.inc"
}

// =============================================================================================
// fused task step
// =============================================================================================

// MODE (compile-time, so the per-step launch carries no loop and none of the reset-only code):
//   MODE_STEP    one step(action) per launch
//   MODE_ROLLOUT n_steps random-action steps per launch (state stays in registers)
//   MODE_RESET   reset() with random placement
//   MODE_REFRESH open a new episode on the state already in the buffers for the envs flagged in
//                the third row of the flags array (reset_to); their observations recomputed, state untouched
// (the constants: rsx_params.hpp)

#ifndef RSX_TASK_KERNEL_ATTR
#define RSX_TASK_KERNEL_ATTR   // (rsx_big.hip sets an occupancy target for its build of this kernel)
#endif
template <int KIND, int L, int TASK, int NR, int MODE>
__global__ __launch_bounds__(64) RSX_TASK_KERNEL_ATTR void task_step_kernel(RSX_HOT_ARGS, const Params P_, const Buffers bufs_) {
    constexpr bool PHYS = false;
    float* const phys = nullptr;
#include "rsx_task_step_body.inc"
}
// the fused step of a physics-enabled handle (rsx_physics_enable): each env with its own coefficients, redrawn at its episode
// starts when a randomisation range is set.  Same launch shape as task_step_kernel, one more argument (the physics block).
template <int KIND, int L, int TASK, int NR, int MODE>
__global__ __launch_bounds__(64) void task_step_phys_kernel(RSX_HOT_ARGS, const Params P_, const Buffers bufs_, float* phys) {
    constexpr bool PHYS = true;
#include "rsx_task_step_body.inc"
}

}  // namespace rsx
