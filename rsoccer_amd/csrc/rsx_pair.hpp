// rsx_pair.hpp — the paired form of the fused single step: task_step_kernel's body (rsx_task_step_body.inc) run by workgroups of TWO
// waves.  Wave 0 is the wave of task_step_kernel and carries the physics chain; wave 1, the service wave, has the same lane ->
// (env, body) map and takes what does not need the physics wave's registers off it (rsx_step_service.inc): the step's random draws
// at the start, the ball lane's reward / info / flags / episode counters at the end.  At the headline batch a launch lasts as long
// as the instruction stream of its slowest wave, and half of the SIMDs are empty: the service wave runs on one of them.
//
// The physics wave's sub-steps (rsx_contact.hpp: physics, rsx_substep_body.inc) take the three sub-step cuts (SubstepCuts: one
// ball-in-flight ballot per step and a loop without the flight gate and the ball-height ballot when every ball of the wave is down,
// the normal impulse by select, the partner prefetch in every iteration): the wave that finishes last walks partners in every sub-step,
// and each exec-mask branch chain it no longer runs there is a stall no other wave covers.  task_step_kernel<0,8,1,6,0> takes the same.
// This kernel alone takes two more: the exchange of every sweep on all lanes and the actuation by select (measured per kernel).
//
// The waves meet at two hardware barriers per step and exchange through LDS (PairBox, and Shared::x0 as before); nothing crosses a
// launch and no array is added.  Results are those of task_step_kernel bit for bit: the same functions on the same floats.
// Which handles run it: rsx_layout.hpp (StepPlan::service_wave).
#pragma once
#include "rsx_kernels.hpp"

namespace rsx {

// what the two waves of a workgroup hand each other besides Shared::x0
struct PairBox {
    float2 dr[64];    // service -> physics, barrier 1: the lane's two draws of this step (draw_for_step, v[0..1]; VSS-v0 has no more)
    float4 ball[8];   // physics -> service, barrier 2: the env's ball after the step and before it: x, y, lastx, lasty
    uint32_t tick;    // physics -> service, device-keyed handles only: the step counter this launch read, and whether it may run
    uint32_t ok;
};

// The workgroup's hardware barrier with LDS-only fences: the wave's DS operations are complete (lgkmcnt) before it arrives and
// none is issued early, and its outstanding global loads and stores stay in flight across it — __syncthreads() would drain them
// (rsx_math.hpp: wave_sync).
__device__ __forceinline__ void pair_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// The physics wave's head (rsx_task_step_body.inc, the line under RSX_PAIR_HEAD): every global load of the wave in front of barrier 1
// is issued in front of ONE wait, one memory round trip instead of two.  -DRSX_PAIR_HEAD=0 on the compiler's line builds the head
// without it for an A/B (tools/build_variant.py).
#ifndef RSX_PAIR_HEAD
#define RSX_PAIR_HEAD 1
#endif

// VSS-v0, eight lanes per env, single steps, literal coefficients: the one variant that is built (rsx_pair.hip)
template <int KIND, int L, int TASK, int NR, int MODE>
__global__ __launch_bounds__(128) void task_pair_step_kernel(RSX_HOT_ARGS, const Params P_, const Buffers bufs_) {
    static_assert(KIND == RSX_KIND_VSS && TASK == RSX_TASK_VSS_V0 && L == 8 && MODE == MODE_STEP, "the paired form exists for the VSS-v0 single step");
    constexpr bool PHYS = false;
    float* const phys = nullptr;
#define RSX_STEP_PAIRED 1
#include "rsx_task_step_body.inc"
#undef RSX_STEP_PAIRED
}

}  // namespace rsx
