// rsx_lane_map.hpp — the lane-group kernels' wave: which lane holds which body of which env (LaneMap), the LDS record the
// lanes of a wave exchange through (Shared), the one-offset-per-lane addressing of the [rows][B] arrays (at_byte) and the
// rare-branch hint.  Needs nothing of the simulator: every other part of the lane-group kernels builds on this one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rsx {

// (the rows of the per-env scalar arena `aux` and the launch argument block `Buffers`: rsx_params.hpp)

// (Observation values go straight from the lane that owns them to the row in HBM — scattered 4-byte stores inside the tile's contiguous
// run of rows — not through an LDS staging area + a coalesced copy-out: measured, VSS-v0 4096 envs 10.01 -> 9.74 us per step,
// 65 536 envs 26.1 -> 25.2; the SSL tasks 0-1 %.)
template <int L>
struct Shared {
    float4 A[64];   // x, y, vx, vy of every body (slot = lane)
    float4 Bq[64];  // SSL robot -> ball record 0: dvx, dvy, dpx, dpy (ball side)
    float4 Cq[64];  // SSL robot -> ball record 1: flags, ovx, ovy, ovz
    float Dq[64];   // SSL robot -> ball record 2: spin change of the ball
    float W[64];    // robots: yaw rate, ball: spin (rad/s) — read on the contact path only
    float2 F[64];   // VSS: held axes of the body in this sweep's snapshot (rsx_body.hpp: held_axes) — read on the contact path only
    alignas(16) float X[64], Y[64];   // positions once more, [env slot][body]: four partners per 16-byte read for the packed overlap test
    float x0[64 / L][12];      // robot 0 -> reward lane exchange
    float2 draws[64 / L][L < 16 ? 16 : L];  // placement: speculative Philox draws of an ended env
    uint32_t ep[64];           // placement helper: the episode ids of the wave's 64 envs
#ifdef RSX_TIMING
    unsigned long long* dbg;   // development builds: where the sub-step stamps go (nullptr = none)
#endif
};

// Marks a branch as seldom taken so that its body is laid out away from the hot path.  Which hints
// pay off was measured per simulator class (single-step launch): SSL takes all three (static
// defenders 10.7 -> 10.5 us, pass endurance 11.2 -> 10.85); VSS takes the contact sweep (2) and
// the episode end (4) but not the airborne-ball test (1): 8.55 -> 8.47 us (all three: 8.62).
#define RSX_RARE_B(KIND, bit, c) (((KIND) == RSX_KIND_SSL || (6 & (bit))) ? __builtin_expect(!!(c), 0) : !!(c))

// Addresses into the [rows][B] arrays on the hot paths: a uniform base pointer (scalar registers) + ONE 32-bit BYTE offset per
// lane — the global_load / global_store "saddr" form, no 64-bit vector multiply-adds and shifts per access.  The host refuses
// batches whose arrays would reach 4 GB (rsx_create / rsx_task_attach: RSX_ERR_ARG).
typedef uint32_t ix_t;
__device__ __forceinline__ float& at_byte(float* base, const ix_t off) { return *reinterpret_cast<float*>(reinterpret_cast<char*>(base) + off); }
__device__ __forceinline__ const float& at_byte(const float* base, const ix_t off) { return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + off); }

// Which lane holds body j of the wave's env g (and which LDS slot: slot = lane).  Body-major (lane = j * G + g: the G lanes
// that own "body j" of neighbouring envs are adjacent, every row access is G * 4 contiguous bytes) for L >= 16; env-major
// (lane = g * L + j: an env's eight bodies are eight adjacent lanes) for L == 8 — measured -1 % at 4096 envs, +2-3 % at 65 536.
// Partners are read through the LDS snapshot in every width (reading them through DPP
// row shifts was measured and dropped: profiles/LABBOOK.md).
template <int L>
struct LaneMap {
    static constexpr int G = 64 / L;
    static constexpr bool EM = L == 8;
    static __device__ __forceinline__ int slot(const int j, const int g) { return EM ? g * L + j : j * G + g; }
    static __device__ __forceinline__ int body(const int lane) { return EM ? lane % L : lane / G; }
    static __device__ __forceinline__ int env(const int lane) { return EM ? lane / L : lane % G; }
};
// lanes of the env in slot g
template <int L>
__device__ __forceinline__ unsigned long long env_lane_mask(const int g) {
    constexpr int G = 64 / L;
    if (LaneMap<L>::EM) return ((1ull << L) - 1ull) << (g * L);
    unsigned long long m = 0;
#pragma unroll
    for (int j = 0; j < L; ++j) m |= 1ull << (j * G);
    return m << g;
}

}  // namespace rsx
