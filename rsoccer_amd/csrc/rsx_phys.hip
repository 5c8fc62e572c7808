// rsx_phys.hip — the per-env physics kernels of librsx_hip.so (include/rsx.h: rsx_physics_*), in a translation unit of their own
// so that the instantiations of the existing kernels in rsx_lanes.hip stay exactly what they were.
//
// A physics-enabled handle always steps with the lane-group kernels (task_step_phys_kernel / sim_step_phys_kernel,
// rsx_kernels.hpp): the same variants rsx_lanes.hip picks for a handle's team sizes and lanes per env, never the one-lane-per-env,
// four-lanes-per-env or large-batch builds.
#include <hip/hip_runtime.h>

#include "rsx.h"
#include "rsx_units.hpp"
#include "rsx_variants.hpp"

namespace rsx {

namespace {

// every env of the block at the defaults (one thread per env)
__global__ void phys_init_kernel(float* __restrict__ blk, const int B, const int S, const int kind, const int ts_ms) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B) return;
    float v[NPHYS], c[NCOEF];
    for (int p = 0; p < NPHYS; ++p) v[p] = (float)phys_default(kind, p);
    derive_coefs(kind, ts_ms, v, c);
    float* const raw = phys_raw(blk);
    float* const co = phys_coef(blk, (size_t)S);
    for (int p = 0; p < NPHYS; ++p) raw[(size_t)p * S + e] = v[p];
    for (int i = 0; i < NCOEF; ++i) co[(size_t)i * S + e] = c[i];
}

// rsx_physics_set: values [NPHYS][vstride] (NaN = keep), mask [B] bytes or null.  An env with an invalid value keeps all of its
// values and is counted in the header's error word.
__global__ void phys_set_kernel(float* __restrict__ blk, const float* __restrict__ vals, const uint8_t* __restrict__ mask,
                                const int B, const int S, const int vstride) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B || (mask && !mask[e])) return;
    PhysHeader* const hd = reinterpret_cast<PhysHeader*>(blk);
    float* const raw = phys_raw(blk);
    float v[NPHYS], c[NCOEF];
    bool ok = true;
    for (int p = 0; p < NPHYS; ++p) {
        const float x = vals[(size_t)p * vstride + e];
        v[p] = x != x ? raw[(size_t)p * S + e] : x;
        ok = ok && phys_valid(hd->kind, p, v[p]);
    }
    if (!ok) { atomicAdd(&hd->err, 1u); return; }
    derive_coefs(hd->kind, hd->ts_ms, v, c);
    float* const co = phys_coef(blk, (size_t)S);
    for (int p = 0; p < NPHYS; ++p) raw[(size_t)p * S + e] = v[p];
    for (int i = 0; i < NCOEF; ++i) co[(size_t)i * S + e] = c[i];
}

// rsx_physics_randomize: the ranges travel as kernel arguments (a captured launch carries its own copy)
struct PhysRanges { float lo[16], hi[16]; uint32_t mask; };
__global__ void phys_ranges_kernel(float* __restrict__ blk, const PhysRanges r) {
    PhysHeader* const hd = reinterpret_cast<PhysHeader*>(blk);
    const int i = threadIdx.x;
    if (i < 16) { hd->lo[i] = r.lo[i]; hd->hi[i] = r.hi[i]; }
    if (i == 0) hd->mask = r.mask;
}

}  // namespace

void launch_task_phys(const Params& P, const Buffers& b, const int L, const int NR, float* phys, const int n_steps, const int mode,
                      hipStream_t s) {
    const int grid = lane_grid(L, P.num_envs);
    with_task(P.task, [&](auto kind, auto task, auto nrs, auto fixed) {
        with_mode(mode, [&](auto m) {
            with_task_variant<task, nrs, fixed, 32>(L, NR, [&](auto l, auto nr) {   // (64 lanes per env: refused by rsx_physics_enable)
                launch_task_hot((task_step_phys_kernel<kind, l, task, nr, m>), {grid}, s, mode_steps(m, n_steps), P, b, phys);
            });
        });
    });
}

void launch_sim_phys(const Params& P, const Buffers& b, const int L, const int NR, float* phys, float* state_out, const int rand_tick,
                     hipStream_t s) {
    const int grid = lane_grid(L, P.num_envs);
    const auto launch = [&](auto kind) {
        with_sim_variant<kind, 32>(L, NR, [&](auto l, auto nr) {
            launch_sim_hot((sim_step_phys_kernel<kind, l, nr>), {grid}, s, state_out, rand_tick, P, b, phys);
        });
    };
    if (P.kind == RSX_KIND_VSS) launch(int_c<RSX_KIND_VSS>{});
    else launch(int_c<RSX_KIND_SSL>{});
}

void launch_phys_init(float* blk, const int B, const int S, const int kind, const int ts_ms, hipStream_t s) {
    rsx_launch(phys_init_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, blk, B, S, kind, ts_ms);
}
void launch_phys_set(float* blk, const float* vals, const uint8_t* mask, const int B, const int S, const int vstride, hipStream_t s) {
    rsx_launch(phys_set_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, blk, vals, mask, B, S, vstride);
}
void launch_phys_ranges(float* blk, const float* lo, const float* hi, const uint32_t mask, hipStream_t s) {
    PhysRanges r{};
    for (int p = 0; p < NPHYS; ++p) { r.lo[p] = lo ? lo[p] : 0.0f; r.hi[p] = hi ? hi[p] : 0.0f; }
    r.mask = mask;
    rsx_launch(phys_ranges_kernel, dim3(1), dim3(64), 0, s, blk, r);
}

}  // namespace rsx
