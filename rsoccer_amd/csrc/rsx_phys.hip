// rsx_phys.hip — the per-env physics kernels of librsx_hip.so (include/rsx.h: rsx_physics_*), in a translation unit of their own
// so that the instantiations of the existing kernels in rsx_api.hip stay exactly what they were.
//
// A physics-enabled handle always steps with the lane-group kernels (task_step_phys_kernel / sim_step_phys_kernel,
// rsx_kernels.hpp): the same variants rsx_api.hip picks for a handle's team sizes and lanes per env, never the one-lane-per-env,
// four-lanes-per-env or large-batch builds.
#include <hip/hip_runtime.h>

#include "rsx_launch.hpp"
#include "rsx.h"
#include "rsx_kernels.hpp"

namespace rsx {

namespace {

dim3 grid_of(const int L, const int B) {   // = grid_for in rsx_api.hip
    const int G = 64 / L;
    const int tiles = (B + G - 1) / G;
    return dim3((unsigned)(((tiles + 7) / 8) * 8));
}

#define RSX_LAUNCH_PHYS(kernel) rsx_launch((kernel), grid, dim3(64), 0, s, b.state, b.aux, b.actions, b.flags, P.num_envs, \
                                           RSX_HOT_DIM(P.state_dim, P.row_stride, P.num_envs), (int)(grid.x >> 3), n_steps, P, b, phys)

template <int KIND, int TASK, int NRS, int MODE>
void task_m(const Params& P, const Buffers& b, const int L, const int NR, float* phys, const int n_steps, hipStream_t s) {
    const dim3 grid = grid_of(L, P.num_envs);
    if (NRS <= 7 && NR == NRS && L == 8) { RSX_LAUNCH_PHYS((task_step_phys_kernel<KIND, 8, TASK, (NRS <= 7 ? NRS : 0), MODE>)); return; }
    if (NRS <= 7 && NR == NRS && L == 16) { RSX_LAUNCH_PHYS((task_step_phys_kernel<KIND, 16, TASK, (NRS <= 7 ? NRS : 0), MODE>)); return; }
    if (TASK == RSX_TASK_SSL_SCRIMMAGE && NR == 22 && L == 32) {
        RSX_LAUNCH_PHYS((task_step_phys_kernel<KIND, 32, TASK, (TASK == RSX_TASK_SSL_SCRIMMAGE ? 22 : 0), MODE>));
        return;
    }
    if (TASK == RSX_TASK_VSS_V0 && NR == 10 && L == 16) {
        RSX_LAUNCH_PHYS((task_step_phys_kernel<KIND, 16, TASK, (TASK == RSX_TASK_VSS_V0 ? 10 : 0), MODE>));
        return;
    }
    switch (L) {   // (64 lanes per env: refused by rsx_physics_enable)
        case 8: RSX_LAUNCH_PHYS((task_step_phys_kernel<KIND, 8, TASK, 0, MODE>)); break;
        case 16: RSX_LAUNCH_PHYS((task_step_phys_kernel<KIND, 16, TASK, 0, MODE>)); break;
        default: RSX_LAUNCH_PHYS((task_step_phys_kernel<KIND, 32, TASK, 0, MODE>)); break;
    }
}
template <int KIND, int TASK, int NRS>
void task_k(const Params& P, const Buffers& b, const int L, const int NR, float* phys, const int n_steps, const int mode, hipStream_t s) {
    switch (mode) {
        case MODE_STEP: task_m<KIND, TASK, NRS, MODE_STEP>(P, b, L, NR, phys, n_steps, s); break;
        case MODE_ROLLOUT: task_m<KIND, TASK, NRS, MODE_ROLLOUT>(P, b, L, NR, phys, n_steps, s); break;
        case MODE_RESET: task_m<KIND, TASK, NRS, MODE_RESET>(P, b, L, NR, phys, 1, s); break;
        default: task_m<KIND, TASK, NRS, MODE_REFRESH>(P, b, L, NR, phys, 1, s); break;
    }
}
// the tasks whose team sizes the task fixes: 8 lanes per env, exact robot count (rsx_api.hip: launch_fixed)
template <int TASK, int NRS, int MODE>
void fixed_m(const Params& P, const Buffers& b, const int L, float* phys, const int n_steps, hipStream_t s) {
    const dim3 grid = grid_of(L, P.num_envs);
    RSX_LAUNCH_PHYS((task_step_phys_kernel<RSX_KIND_SSL, 8, TASK, NRS, MODE>));
}
template <int TASK, int NRS>
void fixed(const Params& P, const Buffers& b, const int L, float* phys, const int n_steps, const int mode, hipStream_t s) {
    switch (mode) {
        case MODE_STEP: fixed_m<TASK, NRS, MODE_STEP>(P, b, L, phys, n_steps, s); break;
        case MODE_ROLLOUT: fixed_m<TASK, NRS, MODE_ROLLOUT>(P, b, L, phys, n_steps, s); break;
        case MODE_RESET: fixed_m<TASK, NRS, MODE_RESET>(P, b, L, phys, 1, s); break;
        default: fixed_m<TASK, NRS, MODE_REFRESH>(P, b, L, phys, 1, s); break;
    }
}

template <int KIND>
void sim_k(const Params& P, const Buffers& b, const int L, const int NR, float* phys, float* state_out, const int rand_tick, hipStream_t s) {
    const dim3 grid = grid_of(L, P.num_envs);
#define RSX_LAUNCH_SIM_PHYS(kernel) rsx_launch((kernel), grid, dim3(64), 0, s, b.state, state_out, b.cmds, b.flags, P.num_envs, \
                                               RSX_HOT_DIM(P.state_dim, P.row_stride, P.num_envs), (int)(grid.x >> 3), rand_tick, P, b, phys)
    if (KIND == RSX_KIND_VSS && NR == 6 && L == 8) { RSX_LAUNCH_SIM_PHYS((sim_step_phys_kernel<KIND, 8, (KIND == RSX_KIND_VSS ? 6 : 0)>)); return; }
    if (KIND == RSX_KIND_VSS && NR == 10) { RSX_LAUNCH_SIM_PHYS((sim_step_phys_kernel<KIND, 16, (KIND == RSX_KIND_VSS ? 10 : 0)>)); return; }
    if (KIND == RSX_KIND_SSL && NR == 7 && L == 8) { RSX_LAUNCH_SIM_PHYS((sim_step_phys_kernel<KIND, 8, (KIND == RSX_KIND_SSL ? 7 : 0)>)); return; }
    if (KIND == RSX_KIND_SSL && NR == 12) { RSX_LAUNCH_SIM_PHYS((sim_step_phys_kernel<KIND, 16, (KIND == RSX_KIND_SSL ? 12 : 0)>)); return; }
    if (KIND == RSX_KIND_SSL && NR == 22) { RSX_LAUNCH_SIM_PHYS((sim_step_phys_kernel<KIND, 32, (KIND == RSX_KIND_SSL ? 22 : 0)>)); return; }
    switch (L) {
        case 8: RSX_LAUNCH_SIM_PHYS((sim_step_phys_kernel<KIND, 8, 0>)); break;
        case 16: RSX_LAUNCH_SIM_PHYS((sim_step_phys_kernel<KIND, 16, 0>)); break;
        default: RSX_LAUNCH_SIM_PHYS((sim_step_phys_kernel<KIND, 32, 0>)); break;
    }
#undef RSX_LAUNCH_SIM_PHYS
}

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
    switch (P.task) {
        case RSX_TASK_VSS_V0: task_k<RSX_KIND_VSS, RSX_TASK_VSS_V0, 6>(P, b, L, NR, phys, n_steps, mode, s); break;
        case RSX_TASK_SSL_STATIC_DEFENDERS: task_k<RSX_KIND_SSL, RSX_TASK_SSL_STATIC_DEFENDERS, 7>(P, b, L, NR, phys, n_steps, mode, s); break;
        case RSX_TASK_SSL_DRIBBLING: fixed<RSX_TASK_SSL_DRIBBLING, 5>(P, b, L, phys, n_steps, mode, s); break;
        case RSX_TASK_SSL_CONTESTED: fixed<RSX_TASK_SSL_CONTESTED, 2>(P, b, L, phys, n_steps, mode, s); break;
        case RSX_TASK_SSL_SCRIMMAGE: case RSX_TASK_SSL_SCRIMMAGE_CROWDED:
            task_k<RSX_KIND_SSL, RSX_TASK_SSL_SCRIMMAGE, 22>(P, b, L, NR, phys, n_steps, mode, s); break;
        default: fixed<RSX_TASK_SSL_PASS_ENDURANCE, 2>(P, b, L, phys, n_steps, mode, s); break;
    }
}

void launch_sim_phys(const Params& P, const Buffers& b, const int L, const int NR, float* phys, float* state_out, const int rand_tick,
                     hipStream_t s) {
    if (P.kind == RSX_KIND_VSS) sim_k<RSX_KIND_VSS>(P, b, L, NR, phys, state_out, rand_tick, s);
    else sim_k<RSX_KIND_SSL>(P, b, L, NR, phys, state_out, rand_tick, s);
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
