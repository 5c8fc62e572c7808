// rsx_lanes.hip — the lane-group kernels of librsx_hip.so (sim_step_kernel, task_step_kernel: 8 / 16 / 32 / 64 lanes per env) and the
// small utility kernels of the C-ABI, in a translation unit of their own: no host-side edit rebuilds them.
//
// Which LAYOUT steps a handle is decided in front of this unit (rsx_layout.hpp, rsx_api_task.hip); what is picked here is the
// variant of the shared table (rsx_variants.hpp) for the handle's team sizes and lanes per env.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rsx.h"
#include "rsx_units.hpp"
#include "rsx_variants.hpp"

using namespace rsx;

namespace {

// debugging aid (rsx_check_finite / RSX_DEBUG_FINITE=1): counts the non-finite floats of a buffer
__global__ void count_nonfinite_kernel(const float* __restrict__ p, size_t n, unsigned long long* out) {
    unsigned long long bad = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        bad += !__builtin_isfinite(p[i]);
    if (bad) atomicAdd(out, bad);
}

// adds the per-block-group partial episode counters into metrics[1..7] and clears them (see metric_slot);
// stream-ordered after the step launches whose counts it collects.  One wave; lane = counter.
__global__ void fold_metrics_kernel(unsigned long long* __restrict__ metrics, unsigned long long* __restrict__ slots) {
    const int i = threadIdx.x;
    if (i < 1 || i >= RSX_METRICS) return;   // metrics[0] (env-steps) is kept by the step kernels directly
    unsigned long long sum = 0;
    for (int s = 0; s < MSLOTS; ++s) { sum += slots[(size_t)s * RSX_METRICS + i]; slots[(size_t)s * RSX_METRICS + i] = 0ull; }
    metrics[i] += sum;
}

template <int KIND>
void launch_sim_k(const Params& P, const Buffers& b, int L, int NR, float* state_out, int rand_tick, hipStream_t s) {
    with_sim_variant<KIND, 64>(L, NR, [&](auto l, auto nr) {
        launch_sim_hot((sim_step_kernel<KIND, l, nr>), {lane_grid(L, P.num_envs)}, s, state_out, rand_tick, P, b);
    });
}

// teleport of rsim.py:52-75 from device arrays: one thread per env, rows are coalesced across threads
__global__ void reset_dev_kernel(float* __restrict__ st, const float* __restrict__ ball, const float* __restrict__ blue,
                                 const float* __restrict__ yellow, const uint8_t* __restrict__ mask, int B, int S_, int rows,
                                 int rs, int nb, int ny, float r_ball) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B || (mask && !mask[e])) return;
    const size_t S = (size_t)S_;   // floats per row
    for (int f = 0; f < rows; ++f) st[(size_t)f * S + e] = 0.0f;
    st[0 * S + e] = ball[4 * (size_t)e + 0]; st[1 * S + e] = ball[4 * (size_t)e + 1]; st[2 * S + e] = r_ball;
    st[3 * S + e] = ball[4 * (size_t)e + 2]; st[4 * S + e] = ball[4 * (size_t)e + 3];
    for (int k = 0; k < nb + ny; ++k) {
        const float* src = k < nb ? blue + ((size_t)e * nb + k) * 3 : yellow + ((size_t)e * ny + (k - nb)) * 3;
        const size_t r = (size_t)(5 + rs * k);
        st[(r + 0) * S + e] = src[0]; st[(r + 1) * S + e] = src[1]; st[(r + 2) * S + e] = src[2];
    }
}

// wire format <-> device layout, for the host-format calls of batches too large for the zero-copy path.  One thread per float64 of the
// wire array (consecutive threads = consecutive addresses of the pinned host buffer: full PCIe packets); the device side of each
// access is a 4-byte piece of an SoA row (absorbed by the L2).
//   commands: wire [B][NC] f64 (rsim.py:92-101 / :129-153)  ->  cmds [NC][S] f32
__global__ void wire_cmds_in_kernel(const double* __restrict__ wire, float* __restrict__ cmds, const unsigned B, const unsigned NC, const unsigned S) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * NC) return;
    const unsigned e = i / NC, j = i - e * NC;
    cmds[(size_t)j * S + e] = (float)wire[i];
}
//   state: state [rows][S] f32  ->  wire [B][rows] f64 (get_state() layout, Entities/Frame.py:20-47 / :55-92, + the two internal rows)
__global__ void wire_state_out_kernel(const float* __restrict__ st, double* __restrict__ wire, const unsigned B, const unsigned rows, const unsigned S) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * rows) return;
    const unsigned e = i / rows, f = i - e * rows;
    wire[i] = (double)st[(size_t)f * S + e];
}

// One launch of the task's lane-group kernels: the variant of the shared table
template <int KIND, int TASK, int NRS, bool FIXED, int MODE>
void launch_task_m(const Params& P, const Buffers& b, int L, int NR, int helpers, int n_steps, hipStream_t s) {
    with_task_variant<TASK, NRS, FIXED, 64>(L, NR, [&](auto l, auto nr) {
        launch_task_hot((task_step_kernel<KIND, l, TASK, nr, MODE>), {lane_grid(L, P.num_envs), helpers}, s, n_steps, P, b);
    });
}

// slots [from, to) := value, or := slot 0 (copy != 0).  Stream-ordered between two stepping launches.
__global__ void tick_fill_kernel(uint32_t* __restrict__ slots, int from, int to, uint32_t value, int copy) {
    const int i = from + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < to) slots[i] = copy ? __atomic_load_n(&slots[0], __ATOMIC_RELAXED) : value;
}

}  // namespace

namespace rsx {

void launch_sim(const Params& P, const Buffers& b, int L, int NR, float* state_out, int rand_tick, hipStream_t s) {
    if (P.kind == RSX_KIND_VSS) launch_sim_k<RSX_KIND_VSS>(P, b, L, NR, state_out, rand_tick, s);
    else launch_sim_k<RSX_KIND_SSL>(P, b, L, NR, state_out, rand_tick, s);
}

void launch_task(const Params& P, const Buffers& b, int L, int NR, int helpers, int n_steps, int mode, hipStream_t s) {
    with_task(P.task, [&](auto kind, auto task, auto nrs, auto fixed) {
        with_mode(mode, [&](auto m) { launch_task_m<kind, task, nrs, fixed, m>(P, b, L, NR, helpers, mode_steps(m, n_steps), s); });
    });
}

void launch_count_nonfinite(const float* p, size_t n, unsigned long long* out, hipStream_t s) {
    rsx_launch(count_nonfinite_kernel, dim3((unsigned)std::clamp<size_t>((n + 255) / 256, 1, 2048)), dim3(256), 0, s, p, n, out);
}
void launch_fold_metrics(unsigned long long* metrics, unsigned long long* slots, hipStream_t s) { rsx_launch(fold_metrics_kernel, dim3(1), dim3(64), 0, s, metrics, slots); }
void launch_reset_dev(float* st, const float* ball, const float* blue, const float* yellow, const uint8_t* mask, int B, int S, int rows, int rs, int nb, int ny,
                      float r_ball, hipStream_t s) {
    rsx_launch(reset_dev_kernel, dim3((B + 255) / 256), dim3(256), 0, s, st, ball, blue, yellow, mask, B, S, rows, rs, nb, ny, r_ball);
}
void launch_wire_cmds_in(const double* wire, float* cmds, unsigned B, unsigned NC, unsigned S, hipStream_t s) {
    rsx_launch(wire_cmds_in_kernel, dim3((B * NC + 255) / 256), dim3(256), 0, s, wire, cmds, B, NC, S);
}
void launch_wire_state_out(const float* st, double* wire, unsigned B, unsigned rows, unsigned S, hipStream_t s) {
    rsx_launch(wire_state_out_kernel, dim3((B * rows + 255) / 256), dim3(256), 0, s, st, wire, B, rows, S);
}
void launch_tick_fill(uint32_t* slots, int from, int to, uint32_t value, int copy, hipStream_t s) {
    if (to > from) rsx_launch(tick_fill_kernel, dim3((unsigned)((to - from + 255) / 256)), dim3(256), 0, s, slots, from, to, value, copy);
}

}  // namespace rsx
#ifdef RSX_TIMING
extern "C" int rsx_dbg_set(unsigned long long* p) { rsx::g_dbg = p; return 0; }   // development builds: s_memtime stamps
#endif
