// rsx_api.hip — host side of librsx_hip.so: the C-ABI declared in include/rsx.h.
//
// Stands where the pybind11 module `robosim` stands in the reference (constructed at
// rsoccer_gym/Simulators/rsim.py:116-124,169-177; stepped at :102,:155; read at :105,:158;
// reset at :38; field at :50; destroyed at :41).  HIP only: there is no CPU path in this library.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "rsx.h"
#include "rsx_units.hpp"
#include "rsx_variants.hpp"

using namespace rsx;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            return fail(RSX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)

}  // namespace

// smallest batch stepped by the one-lane-per-env kernels: measured crossovers of single-step launches (round 3,
// gpurun_out/xover.txt -> profiles/r03_layout_crossovers.txt; multi-step launches cross earlier): VSS-v0 98 304 envs
// (31.5 vs 29.3 us), static defenders 65 536 (29.2 vs 28.5), dribbling 49 152 (30.0 vs 29.2), contested possession
// 32 768 (19.5 vs 18.8), pass endurance 32 768 (17.8 vs 15.3)
#ifndef RSX_EPL_MIN_ENVS
#define RSX_EPL_MIN_ENVS 98304
#endif
// smallest batch of the SSL 11v11 scrimmage task stepped by the large-batch build of its kernel (rsx_big.hip)
#ifndef RSX_BIG_MIN_ENVS
#define RSX_BIG_MIN_ENVS 8192
#endif
// smallest batches of the scrimmage task stepped by the four-lanes-per-env kernel (RSX_LAYOUT=quad|lanes overrides)
#ifndef RSX_QUAD_MIN_ENVS
#define RSX_QUAD_MIN_ENVS 32768
#endif
#ifndef RSX_QUAD_MIN_ENVS_CROWDED
#define RSX_QUAD_MIN_ENVS_CROWDED 65536
#endif
// from this batch on a multi-step call (rsx_task_rollout) on a four-lane handle is issued as single-step launches
#ifndef RSX_QUAD_ROLLOUT_MIN_ENVS
#define RSX_QUAD_ROLLOUT_MIN_ENVS 49152
#endif
#ifndef RSX_QUAD_ROLLOUT_MIN_ENVS_CROWDED
#define RSX_QUAD_ROLLOUT_MIN_ENVS_CROWDED 196608
#endif
#ifndef RSX_EPL_MIN_ENVS_SSL
#define RSX_EPL_MIN_ENVS_SSL 65536
#endif
// largest batch whose single-step launches carry placement-helper workgroups (rsx_kernels.hpp: placement_helper): where a
// launch is as long as its slowest wave and half of the SIMDs are idle anyway
#ifndef RSX_PCACHE_MAX_ENVS
#define RSX_PCACHE_MAX_ENVS 16384
#endif
// largest batch whose host-format step (rsx_step / rsx_step_state) lets the kernel read the commands from, and mirror the
// state into, pinned host memory (one launch + one synchronisation; PCIe latency instead of two copy engines' worth of it)
#ifndef RSX_ZERO_COPY_MAX_ENVS
#define RSX_ZERO_COPY_MAX_ENVS 64
#endif

struct rsx_sim {
    Params P;
    HostModel M;
    int device = 0;
    int field_type = 0, time_step_ms = 0;   // as given to rsx_create (checkpoint header)
    int L = 8;   // lanes per env
    int NR = 0;  // compile-time robot count of the selected kernel variant (0 = generic)
    bool quad = false; // SSL 11v11 scrimmage: single-step launches of a large batch use the four-lanes-per-env kernel (rsx_quad_ssl.hpp)
    bool big = false;  // SSL 11v11 scrimmage: step / rollout launches use the large-batch build of the 32-lane kernel (rsx_big.hip)
    bool epl = false;  // VSS-v0 3v3 / the registered SSL tasks: step and rollout launches use the one-lane-per-env kernels (large batches)
    // one allocation per lifetime stage (few pages -> few TLB entries per launch)
    char* arena_sim = nullptr;   // state | cmds
    char* arena_task = nullptr;  // aux | obs | final_obs | flags | actions | metrics
    float* d_state = nullptr;
    float* d_state_alt = nullptr;   // second state buffer of rsx_step_dev_flip (allocated on first use)
    float* alt_alloc = nullptr;     // ... the allocation behind it: d_state and d_state_alt trade places at every flip, this is what is freed
    float* d_cmds = nullptr;
    float *d_aux = nullptr, *d_obs = nullptr, *d_final_obs = nullptr, *d_actions = nullptr;
    uint8_t* d_flags = nullptr;
    unsigned long long* d_metrics = nullptr;
    unsigned long long* d_mslots = nullptr;   // [MSLOTS][RSX_METRICS] partial episode counters (metric_slot)
    float* d_pcache = nullptr;                // placement cache of the latency-bound batches (rsx_kernels.hpp: placement_helper), or null
    unsigned long long* d_pcstats = nullptr;  // [2] cache hits / inline placements (RSX_PCACHE_STATS=1)
    unsigned long long* d_check = nullptr;   // rsx_check_finite counter
    std::vector<float> h_f32;
    // host-format path: pinned staging; rsx_step() brings the new state back with its own
    // synchronisation, so the rsx_get_state() that follows it (rsim.py:102 then :105) is a pure
    // host conversion.  The copy is trusted only while every state change went through this API:
    // handing out raw device pointers (rsx_dev_view_get) switches the shortcut off for good.
    float* pin_cmds = nullptr;
    float* pin_state = nullptr;
    float* pin_cmds_dev = nullptr;            // the same two buffers as the device sees them (zero-copy path of small batches)
    float* pin_state_dev = nullptr;
    // batches above RSX_ZERO_COPY_MAX_ENVS: the reference's wire format itself (float64, [B][N*C] commands, [B][state_dim + 2] state) in
    // pinned host memory; small kernels convert between it and the f32 SoA arrays ON THE DEVICE, reading / writing the pinned buffers
    // across PCIe — no transposing loop on a CPU thread, no staging copy (rsx_wire_buffers / rsx_step_wire; rsx_step / rsx_get_state
    // are a memcpy in front of / behind them)
    double* wire_cmds = nullptr;
    double* wire_state = nullptr;
    double* wire_cmds_dev = nullptr;
    double* wire_state_dev = nullptr;
    bool host_state_valid = false;
    bool host_state_cache = true;
    bool task_ready = false;   // a reset has opened the first episode
    size_t arena_task_bytes = 0, pcache_bytes = 0;   // sizes of arena_task and of the placement cache inside it (rsx_task_reseed re-initialises them)
    uint32_t tick = 0;                        // fused steps taken since attach (key of the per-step draws); stale once tick_dev is set
    // rsx_task_enable_capture: the step counter lives in device memory (one slot per workgroup behind the metrics vector,
    // rsx_kernels.hpp: step_tick) so that captured stepping launches advance it when a graph replays them
    bool tick_dev = false;
    int tick_slots = 0;                       // workgroups of the handle's per-step launches: the slots every stepping call keeps in sync
    float* d_phys = nullptr;                  // rsx_physics_enable: the per-env physics block (rsx_phys.hpp: PhysHeader, rows), or null
    // rsx_trace_load: one allocation, frames [state_dim + 2][trace_frames] | cmds [N * C][trace_frames - 1] | anchors int32, or null
    float* d_trace = nullptr;
    int trace_frames = 0, trace_anchors = 0, trace_anchor_max = 0;
    size_t trace_cmds_off = 0, trace_anchors_off = 0;   // byte offsets into d_trace
    // rsx_render_open: every view the handle was ever given stays allocated until rsx_destroy (a captured rsx_render holds its view's
    // template pointer in the graph); d_render_err: the error word all of them share.  render_cur: the view rsx_render draws, or -1
    struct RenderSlot {
        rsx_render_view view;
        RenderGeom geom;
        uint8_t* tpl;        // one allocation: field image [H][W][3] | the same as planes [3][H][W]
        size_t tpl_bytes;    // size of each
    };
    std::vector<RenderSlot> render_views;
    int render_cur = -1;
    uint32_t* d_render_err = nullptr;
    // rsx_task_transfer with dst == src: staging records (the per-env arrays once more, addressed by the pair index).  Growing only; a
    // buffer that was outgrown stays allocated until rsx_destroy (a captured same-handle transfer holds its pointer in the graph)
    std::vector<char*> xfer_stage;            // every staging allocation; the last one is current
    int xfer_cap = 0;                         // records the current one holds
    int tick_slots_alloc = 0;                 // slots allocated (the largest grid any layout of this batch could launch): rsx_task_enable_capture and
                                              // rsx_task_checkpoint_load write ALL of them, so that no grid ever reads a slot nobody has set
};

namespace {

int pick_lanes(int n_bodies) {
    int L = n_bodies <= 8 ? 8 : n_bodies <= 16 ? 16 : 32;
    // RSX_LANES_PER_ENV=64 forces the "one wavefront per env" layout (for A/B measurements)
    if (const char* s = std::getenv("RSX_LANES_PER_ENV")) {
        int v = std::atoi(s);
        if ((v == 8 || v == 16 || v == 32 || v == 64) && v >= L) L = v;
    }
    return L;
}

// workgroups of the handle's lane-group launches, and the placement helpers behind them in a single-step launch of a handle
// with a placement cache (rsx_task_attach: 8 lanes per env, exact robot count): one per 64 envs
int grid_for(const rsx_sim* h) { return lane_grid(h->L, h->P.num_envs); }
int helpers_for(const rsx_sim* h, int mode) { return mode == MODE_STEP && h->d_pcache ? (h->P.num_envs + 63) / 64 : 0; }

#ifdef RSX_TIMING
unsigned long long* g_dbg = nullptr;  // development builds: s_memtime stamps
#endif

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

Buffers buffers_of(const rsx_sim* h, const float* actions) {
    Buffers b;
    b.state = h->d_state; b.aux = h->d_aux; b.obs = h->d_obs; b.final_obs = h->d_final_obs;
    b.flags = h->d_flags; b.cmds = h->d_cmds; b.actions = actions; b.metrics = h->d_metrics; b.mslots = h->d_mslots;
    b.pcache = h->d_pcache; b.pcstats = h->d_pcstats;
#ifdef RSX_TIMING
    b.dbg = g_dbg;
#endif
    return b;
}

template <int KIND>
void launch_sim_k(const rsx_sim* h, const Params& P_, float* state_out, int rand_tick, hipStream_t s,
                  const float* cmds_src, float* mirror) {
    Buffers b = buffers_of(h, nullptr);
    if (cmds_src) b.cmds = cmds_src;                      // commands straight from pinned host memory (small batches)
    b.flags = reinterpret_cast<uint8_t*>(mirror);         // the raw step's fourth pointer slot: second copy of the new state, or null
    if (h->d_phys) { launch_sim_phys(P_, b, h->L, h->NR, h->d_phys, state_out, rand_tick, s); return; }
    with_sim_variant<KIND, 64>(h->L, h->NR, [&](auto l, auto nr) {
        launch_sim_hot((sim_step_kernel<KIND, l, nr>), {grid_for(h)}, s, state_out, rand_tick, P_, b);
    });
}

// state_out: where the new state is written (nullptr = in place)
// rand_tick >= 0: commands drawn in the kernel with Philox key `seed` (rsx_step_dev_random)
void launch_sim(const rsx_sim* h, hipStream_t s, float* state_out = nullptr, int rand_tick = -1, uint64_t seed = 0,
                const float* cmds_src = nullptr, float* mirror = nullptr) {
    if (!state_out) state_out = h->d_state;
    Params P = h->P;
    if (rand_tick >= 0) { P.key0 = (uint32_t)seed; P.key1 = (uint32_t)(seed >> 32); P.env_id_base = 0; }
    if (h->P.kind == RSX_KIND_VSS) launch_sim_k<RSX_KIND_VSS>(h, P, state_out, rand_tick, s, cmds_src, mirror);
    else launch_sim_k<RSX_KIND_SSL>(h, P, state_out, rand_tick, s, cmds_src, mirror);
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

// One launch of the handle's task kernels.  First the layout rsx_task_attach chose for the handle's stepping launches (the flags
// imply the team sizes and lanes per env their kernels are built for), then the lane-group variant of the shared table
template <int KIND, int TASK, int NRS, bool FIXED, int MODE>
void launch_task_m(const rsx_sim* h, const float* actions, int n_steps, hipStream_t s) {
    constexpr bool STEPPING = MODE == MODE_STEP || MODE == MODE_ROLLOUT;
    const Buffers b = buffers_of(h, actions);
    if (STEPPING && h->epl) {
        if (TASK == RSX_TASK_VSS_V0) launch_vss_epl(MODE == MODE_ROLLOUT, h->P, b, n_steps, s);
        else launch_ssl_epl(TASK, MODE == MODE_ROLLOUT, h->P, b, n_steps, s);
        return;
    }
    if (MODE == MODE_STEP && h->quad) { launch_ssl_quad(h->P, b, n_steps, s); return; }
    if (STEPPING && h->big) { launch_scrimmage_big(MODE == MODE_ROLLOUT, h->P, b, n_steps, s); return; }
    with_task_variant<TASK, NRS, FIXED, 64>(h->L, h->NR, [&](auto l, auto nr) {
        launch_task_hot((task_step_kernel<KIND, l, TASK, nr, MODE>), {grid_for(h), helpers_for(h, MODE)}, s, n_steps, h->P, b);
    });
}

void launch_task(const rsx_sim* h, const float* actions, int n_steps, int mode, hipStream_t s) {
    actions = mode_actions(mode, actions);
    if (h->d_phys) { launch_task_phys(h->P, buffers_of(h, actions), h->L, h->NR, h->d_phys, n_steps, mode, s); return; }
    with_task(h->P.task, [&](auto kind, auto task, auto nrs, auto fixed) {
        with_mode(mode, [&](auto m) { launch_task_m<kind, task, nrs, fixed, m>(h, actions, mode_steps(m, n_steps), s); });
    });
}

// workgroups of the handle's stepping launches (MODE_STEP / MODE_ROLLOUT), mirroring the dispatch above: what the
// per-workgroup tick slots of a device-keyed handle are sized and kept in sync by (rsx_kernels.hpp: step_tick)
int step_grid(const rsx_sim* h, int mode) {
    const int B = h->P.num_envs;
    if (h->d_phys) return grid_for(h);   // (the per-env physics kernels: tiles only)
    if (h->epl) return epl_grid(B);
    if (h->quad && mode == MODE_STEP) return ssl_quad_grid(B);
    return grid_for(h) + helpers_for(h, mode);
}
uint32_t* tick_words(const rsx_sim* h) { return reinterpret_cast<uint32_t*>(h->d_metrics); }

// slots [from, to) := value, or := slot 0 (copy != 0).  Stream-ordered between two stepping launches.
__global__ void tick_fill_kernel(uint32_t* __restrict__ slots, int from, int to, uint32_t value, int copy) {
    const int i = from + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < to) slots[i] = copy ? __atomic_load_n(&slots[0], __ATOMIC_RELAXED) : value;
}
void tick_fill(const rsx_sim* h, int from, int to, uint32_t value, int copy, hipStream_t s) {
    if (to <= from) return;
    rsx_launch(tick_fill_kernel, dim3((unsigned)((to - from + 255) / 256)), dim3(256), 0, s,
                       tick_words(h) + TICK_SLOT_WORD0, from, to, value, copy);
}

// Makes the handle's device current for the duration of one API call and puts the caller's device
// back on exit: a C-ABI call must not change the thread's current HIP device (which is also
// torch's current device) behind the caller's back.  The per-step calls pay one hipGetDevice.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    int enter(int device) {
        if (hipGetDevice(&prev) == hipSuccess && prev == device) return RSX_OK;
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) return fail(RSX_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
        switched = prev >= 0;
        return RSX_OK;
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

// (kernel launches report through rsx_launch's own record, rsx_launch.hpp — reset on the way in; the thread's HIP last-error slot, which
// the caller's other HIP work shares, is neither read nor cleared here)
#define RSX_ENTER(h)                                              \
    if (!(h)) return fail(RSX_ERR_ARG, "null handle");            \
    DeviceGuard _guard;                                           \
    if (int _rc = _guard.enter((h)->device)) return _rc;          \
    (void)launch_status()

#define RSX_ENTER_TASK(h)                                                                        \
    RSX_ENTER(h);                                                                                \
    (h)->host_state_valid = false; /* every task call may change the state */                    \
    if ((h)->P.task == RSX_TASK_NONE) return fail(RSX_ERR_STATE, "no task attached (rsx_task_attach)")

// stepping before any reset would run on the dummy line-up with episode id 0xFFFFFFFF
#define RSX_NEED_RESET(h) \
    if (!(h)->task_ready) return fail(RSX_ERR_STATE, "rsx_task_reset / rsx_task_reset_to must come before the first step")

// host f64 AoS [B][S'] <-> device f32 SoA [S'][B]
int upload_state(rsx_sim* h, const std::vector<float>& soa, hipStream_t s) {
    h->host_state_valid = false;
    HIP_TRY(hipMemcpyAsync(h->d_state, soa.data(), soa.size() * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    return RSX_OK;
}
int download_state(rsx_sim* h, std::vector<float>& soa, hipStream_t s) {
    soa.resize((size_t)(h->P.state_dim + X_ROWS) * h->P.row_stride);
    HIP_TRY(hipMemcpyAsync(soa.data(), h->d_state, soa.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return RSX_OK;
}

// write the teleport of rsim.py:52-75 into a host SoA copy
void apply_reset(const rsx_sim* h, std::vector<float>& soa, const double* ball, const double* blue,
                 const double* yellow, const uint8_t* mask) {
    const Params& P = h->P;
    const size_t B = (size_t)P.num_envs, S = (size_t)P.row_stride;   // soa: [rows][S], the device layout
    for (size_t e = 0; e < B; ++e) {
        if (mask && !mask[e]) continue;
        for (int f = 0; f < P.state_dim + X_ROWS; ++f) soa[(size_t)f * S + e] = 0.0f;
        const double* bl = ball + 4 * e;
        soa[0 * S + e] = (float)bl[0]; soa[1 * S + e] = (float)bl[1]; soa[2 * S + e] = (float)h->M.field[6];
        soa[3 * S + e] = (float)bl[2]; soa[4 * S + e] = (float)bl[3];
        for (int k = 0; k < P.n_robots; ++k) {
            const double* src = k < P.n_blue ? blue + ((size_t)e * P.n_blue + k) * 3
                                             : yellow + ((size_t)e * P.n_yellow + (k - P.n_blue)) * 3;
            const size_t r = (size_t)(5 + h->M.rs * k);
            soa[(r + 0) * S + e] = (float)src[0];
            soa[(r + 1) * S + e] = (float)src[1];
            soa[(r + 2) * S + e] = (float)src[2];
        }
    }
}

void free_all(rsx_sim* h) {
    if (h->pin_cmds) (void)hipHostFree(h->pin_cmds);
    if (h->pin_state) (void)hipHostFree(h->pin_state);
    h->pin_cmds = h->pin_state = nullptr;
    if (h->wire_cmds) (void)hipHostFree(h->wire_cmds);
    if (h->wire_state) (void)hipHostFree(h->wire_state);
    h->wire_cmds = h->wire_state = nullptr;
    if (h->alt_alloc) (void)hipFree(h->alt_alloc);   // (not d_state_alt: after an odd number of flips that is a pointer INTO arena_sim)
    h->alt_alloc = h->d_state_alt = nullptr;
    if (h->d_check) (void)hipFree(h->d_check);
    h->d_check = nullptr;
    if (h->d_phys) (void)hipFree(h->d_phys);
    h->d_phys = nullptr;
    if (h->d_trace) (void)hipFree(h->d_trace);
    h->d_trace = nullptr;
    for (auto& rv : h->render_views) (void)hipFree(rv.tpl);
    h->render_views.clear(); h->render_cur = -1;
    if (h->d_render_err) (void)hipFree(h->d_render_err);
    h->d_render_err = nullptr;
    for (char* p : h->xfer_stage) (void)hipFree(p);
    h->xfer_stage.clear(); h->xfer_cap = 0;
    if (h->arena_sim) (void)hipFree(h->arena_sim);
    if (h->arena_task) (void)hipFree(h->arena_task);
    h->arena_sim = h->arena_task = nullptr;
}

size_t align_up(size_t n) { return (n + 255) & ~(size_t)255; }

// Floats between the rows of the [rows][B] arrays (state, commands, per-env scalars) beyond B.  With rows exactly B floats apart
// and B a power of two — every batch size anybody benchmarks — row f of an env sits at the same address modulo a large power of
// two for every f, and the ~110 read and write streams of a large-batch launch (one per row) walk the same DRAM banks in step.
// A pad of 64 KB + 256 B per row takes them apart: 4 M envs VSS-v0 150.7 -> 139.3 ps per env-step, 1v6 173.3 -> 150.8; 1 M envs 1v6
// 163.5 -> 152.6; nothing at 262 144 envs and below (the arrays sit in the memory-side cache), where the rows stay dense
// (profiles/r05_row_stride.txt: pads from 256 B to 1 MB; exactly 256 KB is the worst, 64 KB + 256 B and 256 KB + 256 B the best).
// A multiple of 64 floats (rows stay 256-byte aligned; it travels in 16 bits of a hot kernel argument: RSX_HOT_DIM).
// RSX_ROW_PAD=<floats> overrides (tests run every kernel family with padded rows at small batches).
constexpr int RSX_ROW_PAD_MIN_ENVS = 786432;   // (524 288 envs measured: no gain yet)
int row_pad_for(int num_envs) {
    // 64 KB + 256 B up to 1.5 M envs, 256 KB + 256 B beyond: at 2 M envs the smaller pad is no better than none (us per step, pads 0 /
    // 16 448 / 65 600 floats: 1 M envs VSS 164 / 148 / 155, 1v6 169 / 157 / 166; 2 M envs VSS 312 / 314 / 286; 4 M envs VSS 638 / 587 / 585,
    // 1v6 730 / 633 / 623)
    long pad = num_envs < RSX_ROW_PAD_MIN_ENVS ? 0 : num_envs < 1572864 ? 16448 : 65600;
    if (const char* v = std::getenv("RSX_ROW_PAD")) pad = std::atol(v);
    if (pad < 0) pad = 0;
    pad = (pad + 63) / 64 * 64;
    if (pad > 65535l * 64) pad = 65535l * 64;
    return (int)pad;
}

}  // namespace

// state rows, and with a task attached observations, rewards and the cumulative info rows
static int check_finite_impl(rsx_sim* h, int64_t* n_bad, hipStream_t s) {
    if (!h->d_check) HIP_TRY(hipMalloc((void**)&h->d_check, sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(h->d_check, 0, sizeof(unsigned long long), s));
    const size_t B = (size_t)h->P.num_envs, S = (size_t)h->P.row_stride;   // (the pad columns hold zeros)
    auto scan = [&](const float* p, size_t n) {
        const unsigned blocks = (unsigned)std::min<size_t>(2048, (n + 255) / 256);
        rsx_launch(count_nonfinite_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, s, p, n, h->d_check);
    };
    scan(h->d_state, (size_t)(h->P.state_dim + X_ROWS) * S);
    if (h->P.task != RSX_TASK_NONE) {
        scan(h->d_obs, B * (size_t)h->P.obs_dim);
        scan(h->d_aux + (size_t)ROW_REWARD * S, B);
        scan(h->d_aux + (size_t)ROW_INFO * S, S * (size_t)h->M.info_dim);
    }
    HIP_TRY(launch_status());
    unsigned long long bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, h->d_check, sizeof(bad), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *n_bad = (int64_t)bad;
    return RSX_OK;
}

// RSX_DEBUG_FINITE=1: every stepping call is followed by the scan (synchronous: a debugging mode)
static int debug_finite(rsx_sim* h, hipStream_t s, const char* where) {
    static const bool on = std::getenv("RSX_DEBUG_FINITE") != nullptr && std::getenv("RSX_DEBUG_FINITE")[0] == '1';
    if (!on) return RSX_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) (void)hipGetLastError();
    else if (cs != hipStreamCaptureStatusNone) return fail(RSX_ERR_STATE, "RSX_DEBUG_FINITE=1 scans synchronously and cannot run inside a stream capture");
    int64_t bad = 0;
    if (int rc = check_finite_impl(h, &bad, s)) return rc;
    if (bad) return fail(RSX_ERR_STATE, std::string("RSX_DEBUG_FINITE: ") + std::to_string(bad) + " non-finite value(s) after " + where);
    return RSX_OK;
}

extern "C" {

#ifdef RSX_TIMING
int rsx_dbg_set(unsigned long long* p) { g_dbg = p; return 0; }
#endif

int rsx_abi_version(void) { return RSX_ABI_VERSION; }
const char* rsx_last_error(void) { return g_err.c_str(); }

int rsx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rsx_create(rsx_sim** out, int kind, int field_type, int n_blue, int n_yellow, int time_step_ms,
               int num_envs, int device_id) {
    if (!out) return fail(RSX_ERR_ARG, "out is null");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(RSX_ERR_NO_DEVICE, "no HIP device visible: librsx_hip has no CPU path");
    if (device_id < 0 || device_id >= ndev) return fail(RSX_ERR_ARG, "device_id out of range");
    rsx_sim* h = new rsx_sim();
    if (derive_model(kind, field_type, n_blue, n_yellow, time_step_ms, num_envs, h->P, h->M)) {
        delete h;
        return fail(RSX_ERR_ARG, "bad simulator configuration (kind / field_type / robot counts / time step / num_envs)");
    }
    h->P.row_stride = num_envs + row_pad_for(num_envs);
    h->device = device_id;
    h->field_type = field_type; h->time_step_ms = time_step_ms;
    h->L = pick_lanes(h->P.n_robots + 1);
    h->NR = specialised_robots(h->P.kind, h->P.n_robots, h->P.n_blue, h->L);
    auto bail = [&](hipError_t e, const char* what) {
        std::string m = std::string(what) + ": " + hipGetErrorString(e);
        free_all(h); delete h;
        return fail(RSX_ERR_HIP, m);
    };
    hipError_t e;
    DeviceGuard guard;
    if (guard.enter(device_id)) { free_all(h); delete h; return RSX_ERR_HIP; }
    const size_t B = (size_t)num_envs, S = (size_t)h->P.row_stride;
    const size_t sbytes = (size_t)(h->P.state_dim + X_ROWS) * S * sizeof(float);
    const size_t cbytes = (size_t)h->P.n_robots * h->M.cmd_dim * S * sizeof(float);
    if (sbytes >= ((size_t)1 << 32)) {   // the kernels address a row of the state with a 32-bit byte offset (rsx_kernels.hpp: at_byte)
        free_all(h); delete h;
        return fail(RSX_ERR_ARG, "num_envs too large: the state array would reach 4 GB (see rsx.h, limits)");
    }
    if ((e = hipMalloc((void**)&h->arena_sim, align_up(sbytes) + align_up(cbytes))) != hipSuccess) return bail(e, "hipMalloc(state+cmds)");
    h->d_state = (float*)h->arena_sim;
    h->d_cmds = (float*)(h->arena_sim + align_up(sbytes));
    if ((e = hipMemset(h->d_cmds, 0, cbytes)) != hipSuccess) return bail(e, "hipMemset(cmds)");
    if ((e = hipHostMalloc((void**)&h->pin_cmds, cbytes ? cbytes : 4, hipHostMallocDefault)) != hipSuccess) return bail(e, "hipHostMalloc(cmds)");
    if ((e = hipHostMalloc((void**)&h->pin_state, sbytes, hipHostMallocDefault)) != hipSuccess) return bail(e, "hipHostMalloc(state)");
    if (num_envs > RSX_ZERO_COPY_MAX_ENVS && !std::getenv("RSX_NO_WIRE_PATH")) {
        // larger batches: pinned buffers in the wire format, converted on the device (see rsx_sim::wire_cmds)
        const size_t wc = B * (size_t)h->P.n_robots * h->M.cmd_dim * sizeof(double), ws = B * (size_t)(h->P.state_dim + X_ROWS) * sizeof(double);
        void *dc = nullptr, *ds = nullptr;
        if (B * (size_t)(h->P.state_dim + X_ROWS) < ((size_t)1 << 32) &&
            hipHostMalloc((void**)&h->wire_cmds, wc, hipHostMallocDefault) == hipSuccess &&
            hipHostMalloc((void**)&h->wire_state, ws, hipHostMallocDefault) == hipSuccess &&
            hipHostGetDevicePointer(&dc, h->wire_cmds, 0) == hipSuccess && hipHostGetDevicePointer(&ds, h->wire_state, 0) == hipSuccess) {
            h->wire_cmds_dev = (double*)dc; h->wire_state_dev = (double*)ds;
        } else {   // no pinned memory to be had, or not addressable by the device: the staging path below still works
            (void)hipGetLastError();
            if (h->wire_cmds) (void)hipHostFree(h->wire_cmds);
            if (h->wire_state) (void)hipHostFree(h->wire_state);
            h->wire_cmds = h->wire_state = nullptr;
        }
    }
    if (num_envs <= RSX_ZERO_COPY_MAX_ENVS && !std::getenv("RSX_NO_ZERO_COPY")) {
        // small batches (the robosim-shaped single-env objects): the raw step reads its commands from, and mirrors the
        // new state into, the pinned host buffers directly — if the device can address them
        void *dc = nullptr, *ds = nullptr;
        if (hipHostGetDevicePointer(&dc, h->pin_cmds, 0) == hipSuccess && hipHostGetDevicePointer(&ds, h->pin_state, 0) == hipSuccess) {
            h->pin_cmds_dev = (float*)dc; h->pin_state_dev = (float*)ds;
        } else {
            (void)hipGetLastError();
        }
    }
    // the adapter's dummy line-up, rsim.py:20-24
    std::vector<float> soa((size_t)(h->P.state_dim + X_ROWS) * S, 0.0f);
    for (size_t i = 0; i < B; ++i) {
        soa[2 * S + i] = (float)h->M.field[6];
        for (int k = 0; k < h->P.n_robots; ++k) {
            const int j = k < n_blue ? k + 1 : k - n_blue + 1;
            soa[(size_t)(5 + h->M.rs * k) * S + i] = (float)((k < n_blue ? -0.2 : 0.2) * j);
        }
    }
    if ((e = hipMemcpy(h->d_state, soa.data(), sbytes, hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy(state)");
    // the memsets above ran on the null stream; callers step on their own (possibly non-blocking)
    // streams, which do not order themselves behind it
    if ((e = hipDeviceSynchronize()) != hipSuccess) return bail(e, "hipDeviceSynchronize");
    *out = h;
    return RSX_OK;
}

int rsx_destroy(rsx_sim* h) {
    if (!h) return RSX_OK;
    DeviceGuard guard;
    (void)guard.enter(h->device);
    free_all(h);
    delete h;
    return RSX_OK;
}

int rsx_get_field_params(const rsx_sim* h, double out[RSX_FIELD_PARAMS]) {
    if (!h || !out) return fail(RSX_ERR_ARG, "null argument");
    std::memcpy(out, h->M.field, sizeof(double) * RSX_FIELD_PARAMS);
    return RSX_OK;
}

int rsx_reset(rsx_sim* h, const double* ball, const double* blue, const double* yellow,
              const uint8_t* env_mask, void* stream) {
    RSX_ENTER(h);
    if (!ball || (h->P.n_blue && !blue) || (h->P.n_yellow && !yellow)) return fail(RSX_ERR_ARG, "null placement array");
    hipStream_t s = (hipStream_t)stream;
    std::vector<float> soa;
    if (env_mask) { if (int rc = download_state(h, soa, s)) return rc; }
    else soa.assign((size_t)(h->P.state_dim + X_ROWS) * h->P.row_stride, 0.0f);
    apply_reset(h, soa, ball, blue, yellow, env_mask);
    return upload_state(h, soa, s);
}

// the wire-format step of a large batch: commands from h->wire_cmds, new state into h->wire_state (when the host copy is trusted)
static int step_wire_impl(rsx_sim* h, hipStream_t s) {
    const Params& P = h->P;
    const unsigned B = (unsigned)P.num_envs, S = (unsigned)P.row_stride, NC = (unsigned)(P.n_robots * h->M.cmd_dim), rows = (unsigned)(P.state_dim + X_ROWS);
    h->host_state_valid = false;
    rsx_launch(wire_cmds_in_kernel, dim3((B * NC + 255) / 256), dim3(256), 0, s, h->wire_cmds_dev, h->d_cmds, B, NC, S);
    launch_sim(h, s);
    if (h->host_state_cache)
        rsx_launch(wire_state_out_kernel, dim3((B * rows + 255) / 256), dim3(256), 0, s, h->d_state, h->wire_state_dev, B, rows, S);
    HIP_TRY(launch_status());
    HIP_TRY(hipStreamSynchronize(s));
    h->host_state_valid = h->host_state_cache;
    return RSX_OK;
}

int rsx_wire_buffers(rsx_sim* h, double** cmds, double** state) {
    if (!h) return fail(RSX_ERR_ARG, "null handle");
    if (!h->wire_cmds) return fail(RSX_ERR_STATE, "this handle has no wire-format buffers (batches of at most 64 envs step through rsx_step_state without copies)");
    if (cmds) *cmds = h->wire_cmds;
    if (state) *state = h->wire_state;
    return RSX_OK;
}

int rsx_step_wire(rsx_sim* h, void* stream) {
    RSX_ENTER(h);
    if (!h->wire_cmds) return fail(RSX_ERR_STATE, "this handle has no wire-format buffers (rsx_wire_buffers)");
    if (!h->host_state_cache) {   // a device view was handed out: nothing mirrors the state unasked any more, but this call promises it
        h->host_state_cache = true;
        const int rc = step_wire_impl(h, (hipStream_t)stream);
        h->host_state_cache = false; h->host_state_valid = false;
        return rc;
    }
    return step_wire_impl(h, (hipStream_t)stream);
}

int rsx_step(rsx_sim* h, const double* cmds, void* stream) {
    RSX_ENTER(h);
    if (!cmds) return fail(RSX_ERR_ARG, "cmds is null");
    hipStream_t s = (hipStream_t)stream;
    const Params& P = h->P;
    const size_t B = (size_t)P.num_envs, S = (size_t)P.row_stride, NC = (size_t)P.n_robots * h->M.cmd_dim;
    if (h->wire_cmds) {   // large batch: one contiguous copy into the pinned wire buffer, the conversion runs on the device
        if (cmds != h->wire_cmds) std::memcpy(h->wire_cmds, cmds, B * NC * sizeof(double));
        return step_wire_impl(h, s);
    }
    for (size_t e = 0; e < B; ++e)
        for (size_t j = 0; j < NC; ++j) h->pin_cmds[j * S + e] = (float)cmds[e * NC + j];
    h->host_state_valid = false;
    if (h->pin_cmds_dev) {   // small batch: no copies, the kernel talks to the pinned buffers
        launch_sim(h, s, nullptr, -1, 0, h->pin_cmds_dev, h->host_state_cache ? h->pin_state_dev : nullptr);
        HIP_TRY(launch_status());
    } else {
        HIP_TRY(hipMemcpyAsync(h->d_cmds, h->pin_cmds, NC * S * sizeof(float), hipMemcpyHostToDevice, s));
        launch_sim(h, s);
        HIP_TRY(launch_status());
        if (h->host_state_cache)
            HIP_TRY(hipMemcpyAsync(h->pin_state, h->d_state, (size_t)(P.state_dim + X_ROWS) * S * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    h->host_state_valid = h->host_state_cache;
    return RSX_OK;
}

static int get_state_impl(rsx_sim* h, double* out, int rows, hipStream_t s) {
    const size_t B = (size_t)h->P.num_envs, S = (size_t)h->P.row_stride;
    if (h->wire_state) {   // large batch: the wire-format copy is made on the device; what is left is a copy out of pinned memory
        const int all = h->P.state_dim + X_ROWS;
        if (!h->host_state_valid) {
            rsx_launch(wire_state_out_kernel, dim3(((unsigned)B * all + 255) / 256), dim3(256), 0, s, h->d_state, h->wire_state_dev, (unsigned)B, (unsigned)all, (unsigned)S);
            HIP_TRY(launch_status());
            HIP_TRY(hipStreamSynchronize(s));
            h->host_state_valid = h->host_state_cache;
        }
        if (out == h->wire_state) return RSX_OK;
        if (rows == all) std::memcpy(out, h->wire_state, B * (size_t)all * sizeof(double));
        else for (size_t e = 0; e < B; ++e) std::memcpy(out + e * rows, h->wire_state + e * all, (size_t)rows * sizeof(double));
        return RSX_OK;
    }
    if (!h->host_state_valid) {
        HIP_TRY(hipMemcpyAsync(h->pin_state, h->d_state, (size_t)(h->P.state_dim + X_ROWS) * S * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        h->host_state_valid = h->host_state_cache;
    }
    const float* soa = h->pin_state;
    for (size_t e = 0; e < B; ++e)
        for (int f = 0; f < rows; ++f) out[e * rows + f] = (double)soa[(size_t)f * S + e];
    return RSX_OK;
}

int rsx_get_state(rsx_sim* h, double* out, void* stream) {
    RSX_ENTER(h);
    if (!out) return fail(RSX_ERR_ARG, "out is null");
    return get_state_impl(h, out, h->P.state_dim, (hipStream_t)stream);
}

int rsx_step_state(rsx_sim* h, const double* cmds, double* state_out, void* stream) {
    if (!state_out) return fail(RSX_ERR_ARG, "state_out is null");
    if (int rc = rsx_step(h, cmds, stream)) return rc;
    return rsx_get_state(h, state_out, stream);
}

int rsx_get_state_full(rsx_sim* h, double* out, void* stream) {
    RSX_ENTER(h);
    if (!out) return fail(RSX_ERR_ARG, "out is null");
    return get_state_impl(h, out, h->P.state_dim + X_ROWS, (hipStream_t)stream);
}

int rsx_set_state(rsx_sim* h, const double* state, void* stream) {
    RSX_ENTER(h);
    if (!state) return fail(RSX_ERR_ARG, "state is null");
    const size_t B = (size_t)h->P.num_envs, S = (size_t)h->P.row_stride;
    const int rows = h->P.state_dim + X_ROWS;
    std::vector<float> soa((size_t)rows * S);   // (zeros in the pad columns)
    for (size_t e = 0; e < B; ++e)
        for (int f = 0; f < rows; ++f) soa[(size_t)f * S + e] = (float)state[e * rows + f];
    return upload_state(h, soa, (hipStream_t)stream);
}

int rsx_dev_view_get(rsx_sim* h, rsx_dev_view* out) {
    if (!h || !out) return fail(RSX_ERR_ARG, "null argument");
    out->num_envs = h->P.num_envs; out->n_robots = h->P.n_robots;
    out->state_dim = h->P.state_dim; out->cmd_dim = h->M.cmd_dim;
    out->state = h->d_state; out->cmds = h->d_cmds; out->row_stride = h->P.row_stride;
    h->host_state_cache = false; h->host_state_valid = false;   // the caller can now write the state behind our back
    return RSX_OK;
}

int rsx_step_dev(rsx_sim* h, void* stream) {
    RSX_ENTER(h);
    h->host_state_valid = false;
    launch_sim(h, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return debug_finite(h, (hipStream_t)stream, "rsx_step_dev");
}

static int ensure_alt(rsx_sim* h) {
    if (h->d_state_alt) return RSX_OK;
    const size_t sbytes = (size_t)(h->P.state_dim + X_ROWS) * h->P.row_stride * sizeof(float);
    HIP_TRY(hipMalloc((void**)&h->alt_alloc, sbytes));
    h->d_state_alt = h->alt_alloc;
    HIP_TRY(hipMemset(h->d_state_alt, 0, sbytes));
    HIP_TRY(hipDeviceSynchronize());
    return RSX_OK;
}

int rsx_state_buffers(rsx_sim* h, float** current, float** other) {
    RSX_ENTER(h);
    if (!current || !other) return fail(RSX_ERR_ARG, "null argument");
    if (int rc = ensure_alt(h)) return rc;
    *current = h->d_state; *other = h->d_state_alt;
    h->host_state_cache = false; h->host_state_valid = false;
    return RSX_OK;
}

int rsx_step_dev_random(rsx_sim* h, int n, uint64_t seed, uint32_t first_tick, void* stream) {
    RSX_ENTER(h);
    if (n < 1) return fail(RSX_ERR_ARG, "n must be >= 1");
    if ((uint64_t)first_tick + (uint64_t)n > 0x7FFFFFFFull) return fail(RSX_ERR_ARG, "tick range exceeds 2^31");
    h->host_state_valid = false;
    for (int i = 0; i < n; ++i) launch_sim(h, (hipStream_t)stream, nullptr, (int)(first_tick + (uint32_t)i), seed);
    HIP_TRY(launch_status());
    return debug_finite(h, (hipStream_t)stream, "rsx_step_dev_random");
}

int rsx_step_dev_flip(rsx_sim* h, void* stream) {
    RSX_ENTER(h);
    {   // which buffer is current is host state: a replayed graph would keep writing the same one
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) (void)hipGetLastError();
        else if (cs != hipStreamCaptureStatusNone) return fail(RSX_ERR_STATE, "rsx_step_dev_flip cannot be captured (the buffer roles are host state); capture rsx_step_dev instead");
    }
    if (int rc = ensure_alt(h)) return rc;
    h->host_state_valid = false;
    launch_sim(h, (hipStream_t)stream, h->d_state_alt);
    HIP_TRY(launch_status());
    std::swap(h->d_state, h->d_state_alt);
    return debug_finite(h, (hipStream_t)stream, "rsx_step_dev_flip");
}

int rsx_reset_dev(rsx_sim* h, const float* ball_dev, const float* blue_dev, const float* yellow_dev,
                  const uint8_t* env_mask_dev, void* stream) {
    RSX_ENTER(h);
    if (!ball_dev || (h->P.n_blue && !blue_dev) || (h->P.n_yellow && !yellow_dev)) return fail(RSX_ERR_ARG, "null placement array");
    h->host_state_valid = false;
    const int B = h->P.num_envs;
    rsx_launch(reset_dev_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->d_state, ball_dev, blue_dev,
                       yellow_dev, env_mask_dev, B, h->P.row_stride, h->P.state_dim + X_ROWS, h->M.rs, h->P.n_blue, h->P.n_yellow, (float)h->M.field[6]);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_task_attach(rsx_sim* h, int task, uint64_t seed, uint64_t env_id_base, int max_episode_steps) {
    RSX_ENTER(h);
    if (h->P.task != RSX_TASK_NONE) return fail(RSX_ERR_STATE, "a task is already attached");
    // global env ids are 32-bit words of the Philox counter: the whole range of this handle has to fit
    if (env_id_base > 0xFFFFFFFFull || env_id_base + (uint64_t)h->P.num_envs > 0x100000000ull)
        return fail(RSX_ERR_ARG, "env_id_base + num_envs exceeds 2^32 (global env ids are 32-bit)");
    Params P = h->P;
    if (derive_task(task, seed, env_id_base, max_episode_steps, h->M, P))
        return fail(RSX_ERR_ARG, "task does not match the simulator (VSS_V0: VSS, n_blue >= 1; STATIC_DEFENDERS: SSL 1vN; DRIBBLING: SSL 1v4; CONTESTED: SSL 1v1; PASS_ENDURANCE: SSL 2v0; SCRIMMAGE: SSL)");
    if (P.obs_dim > 64) return fail(RSX_ERR_ARG, "observation wider than 64 floats is not supported");
    if (task >= RSX_TASK_SSL_DRIBBLING && task <= RSX_TASK_SSL_PASS_ENDURANCE && h->L != 8)
        return fail(RSX_ERR_ARG, "this task runs with 8 lanes per env only (unset RSX_LANES_PER_ENV)");
    const size_t B = (size_t)P.num_envs, S = (size_t)P.row_stride;
    const size_t n_aux = align_up((size_t)aux_rows(P.n_robots) * S * sizeof(float));
    if (n_aux >= ((size_t)1 << 32) || B * (size_t)P.obs_dim * sizeof(float) >= ((size_t)1 << 32))
        return fail(RSX_ERR_ARG, "num_envs too large for a fused task: the per-env scalar arena or the observation array would reach 4 GB (see rsx.h, limits)");
    const size_t n_obs = align_up(B * P.obs_dim * sizeof(float));
    const size_t n_flags = align_up(3 * B);   // terminated | truncated | the env mask of rsx_task_reset_to (read by the MODE_REFRESH launch only)
    const size_t n_act = align_up(B * h->M.act_dim * sizeof(float));
    // metrics[8] | error word | (256 bytes in) one step-counter slot per workgroup of the largest stepping launch any layout
    // of this batch could use (rsx_kernels.hpp: step_tick; only the first tick_slots are kept in sync)
    const size_t n_met = align_up((size_t)TICK_SLOT_WORD0 * 4 + ((size_t)grid_for(h) + (B + 63) / 64) * sizeof(uint32_t));
    const size_t n_slots = align_up((size_t)MSLOTS * RSX_METRICS * sizeof(unsigned long long));
    // placement cache: static defenders 1v6 (short episodes: several resetting waves per launch) at latency-bound batches
    const bool pc = !std::getenv("RSX_NO_PCACHE") && h->L == 8 && P.num_envs <= RSX_PCACHE_MAX_ENVS && P.n_sub > 0 &&
                    task == RSX_TASK_SSL_STATIC_DEFENDERS && h->NR == 7;
    const size_t n_pc = pc ? align_up((size_t)2 * (3 * (P.n_robots + 1) + 1) * B * sizeof(float)) : 0;
    const size_t n_pcs = pc && std::getenv("RSX_PCACHE_STATS") ? align_up(2 * sizeof(unsigned long long)) : 0;
    const size_t total = n_aux + 2 * n_obs + n_flags + n_act + n_met + n_slots + n_pc + n_pcs;
    HIP_TRY(hipMalloc((void**)&h->arena_task, total));
    HIP_TRY(hipMemset(h->arena_task, 0, total));
    h->arena_task_bytes = total; h->pcache_bytes = n_pc;
    char* p = h->arena_task;
    h->d_aux = (float*)p; p += n_aux;
    h->d_obs = (float*)p; p += n_obs;
    h->d_final_obs = (float*)p; p += n_obs;
    h->d_flags = (uint8_t*)p; p += n_flags;
    h->d_actions = (float*)p; p += n_act;
    h->d_metrics = (unsigned long long*)p; p += n_met;
    h->d_mslots = (unsigned long long*)p; p += n_slots;
    if (n_pc) {
        h->d_pcache = (float*)p; p += n_pc;
        HIP_TRY(hipMemset(h->d_pcache, 0xFF, n_pc));   // tags 0xFFFFFFFF: no entry is valid yet
    }
    if (n_pcs) h->d_pcstats = (unsigned long long*)p;
    // episode ids start at 0xFFFFFFFF so that the first reset() opens episode 0
    HIP_TRY(hipMemset(h->d_aux + (size_t)ROW_EPISODE * S, 0xFF, B * sizeof(uint32_t)));
    h->P = P;
    // The five registered tasks: which tile layout steps the envs.  Both give identical results; the one-lane-
    // per-env kernel needs enough envs to fill the chip with its long waves.
    h->epl = false;
    h->big = false; h->quad = false;
    if ((task == RSX_TASK_SSL_SCRIMMAGE || task == RSX_TASK_SSL_SCRIMMAGE_CROWDED) && h->NR == 22 && h->L == 32) {
        h->big = P.num_envs >= RSX_BIG_MIN_ENVS;
        // four lanes per env: 32-bit row offsets (arrays below 2 GB), a real time step (the infrared row is rewritten)
        const char* lay = std::getenv("RSX_LAYOUT");
        const size_t rows = (size_t)std::max(P.state_dim + X_ROWS, aux_rows(P.n_robots));
        const bool fits = rows * (size_t)P.row_stride * sizeof(float) < ((size_t)1 << 31) && P.n_sub > 0 && P.n_blue == 11;
        // measured crossovers (profiles/LABBOOK.md): the spread line-up from 32 768 envs, the crowded one (contacts in every
        // sub-step: the six robots of a lane are walked one after the other) from 65 536 (RSX_QUAD_MIN_ENVS_CROWDED);
        // multi-step calls on a crowded handle stay with the 32-lane kernel below 262 144 envs (rsx_task_rollout)
        const int quad_min = task == RSX_TASK_SSL_SCRIMMAGE ? RSX_QUAD_MIN_ENVS : RSX_QUAD_MIN_ENVS_CROWDED;
        h->quad = fits && (lay ? std::strcmp(lay, "quad") == 0 : (quad_min > 0 && P.num_envs >= quad_min));
    }
    const bool fixed_ssl = task == RSX_TASK_SSL_DRIBBLING || task == RSX_TASK_SSL_CONTESTED || task == RSX_TASK_SSL_PASS_ENDURANCE;   // team sizes checked above
    if ((task == RSX_TASK_VSS_V0 && h->NR == 6 && h->L == 8) || (task == RSX_TASK_SSL_STATIC_DEFENDERS && h->NR == 7 && h->L == 8) || fixed_ssl) {
        const char* lay = std::getenv("RSX_LAYOUT");
        if (lay && std::strcmp(lay, "epl") == 0) h->epl = true;
        else if (lay && std::strcmp(lay, "lanes") == 0) h->epl = false;
        else h->epl = P.num_envs >= (task == RSX_TASK_VSS_V0 ? RSX_EPL_MIN_ENVS : task == RSX_TASK_SSL_STATIC_DEFENDERS ? RSX_EPL_MIN_ENVS_SSL
                                     : task == RSX_TASK_SSL_DRIBBLING ? 49152 : 32768);
        // those kernels address rows with 32-bit byte offsets (buffer instructions): arrays of 2 GB and more stay with the lane-group kernels
        const size_t rows = (size_t)std::max(P.state_dim + X_ROWS, aux_rows(P.n_robots));
        if (rows * (size_t)P.row_stride * sizeof(float) >= ((size_t)1 << 31) || (size_t)P.num_envs * P.obs_dim * sizeof(float) >= ((size_t)1 << 31)) h->epl = false;
    }
    if (h->d_phys) h->epl = h->big = h->quad = false;   // per-env physics: the lane-group kernels at every batch size
    h->task_ready = false;
    h->tick_dev = false;
    h->tick_slots = step_grid(h, MODE_STEP);
    h->tick_slots_alloc = std::max(h->tick_slots, grid_for(h) + (P.num_envs + 63) / 64);
    HIP_TRY(hipDeviceSynchronize());   // null-stream memsets done before any caller stream steps
    return RSX_OK;
}

int rsx_drop_pending_hip_error(void) { return (int)hipGetLastError(); }

int rsx_task_reseed(rsx_sim* h, uint64_t seed, void* stream) {
    RSX_ENTER_TASK(h);
    hipStream_t s = (hipStream_t)stream;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) (void)hipGetLastError();
    else if (cs != hipStreamCaptureStatusNone) return fail(RSX_ERR_STATE, "rsx_task_reseed changes host state (seed, step counter) and cannot be captured");
    // what rsx_task_attach leaves behind, with the new key: every per-env buffer and counter cleared, episode ids at 0xFFFFFFFF,
    // placement cache empty, step counter 0 (device-keyed handles: every slot), no episode open
    HIP_TRY(hipMemsetAsync(h->arena_task, 0, h->arena_task_bytes, s));
    if (h->d_pcache) HIP_TRY(hipMemsetAsync(h->d_pcache, 0xFF, h->pcache_bytes, s));
    HIP_TRY(hipMemsetAsync(h->d_aux + (size_t)ROW_EPISODE * h->P.row_stride, 0xFF, (size_t)h->P.num_envs * sizeof(uint32_t), s));
    h->P.key0 = (uint32_t)seed; h->P.key1 = (uint32_t)(seed >> 32);
    h->tick = 0; h->P.tick_base = 0;
    h->task_ready = false;
    return RSX_OK;
}

int rsx_task_enable_capture(rsx_sim* h, void* stream) {
    RSX_ENTER_TASK(h);
    // The one place where the thread's pending HIP error is dropped: the usual way to get here is a capture attempt that this library
    // refused (host-keyed handle) and that the caller's framework then aborted — which leaves `invalid argument` in the slot for the
    // NEXT capture to trip over (torch.cuda.graph does).  A set-up call, not a stepping path; rsx.h says so.
    (void)hipGetLastError();
    if (h->tick_dev) return RSX_OK;
    hipStream_t s = (hipStream_t)stream;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) (void)hipGetLastError();
    else if (cs != hipStreamCaptureStatusNone)
        return fail(RSX_ERR_STATE, "rsx_task_enable_capture must be called BEFORE the capture begins (it writes the step counter once; a captured write would reset it on every replay)");
    tick_fill(h, 0, h->tick_slots_alloc, h->tick, 0, s);
    HIP_TRY(launch_status());
    h->tick_dev = true;
    h->host_state_cache = false; h->host_state_valid = false;   // a replayed graph changes the state without passing through this API
    return RSX_OK;
}

int rsx_task_tick(rsx_sim* h, uint32_t* out, void* stream) {
    RSX_ENTER(h);
    if (!out) return fail(RSX_ERR_ARG, "out is null");
    if (h->P.task == RSX_TASK_NONE) return fail(RSX_ERR_STATE, "no task attached (rsx_task_attach)");
    if (!h->tick_dev) { *out = h->tick; return RSX_OK; }
    uint32_t w[2] = {0, 0};   // slot 0, error word
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(&w[0], tick_words(h) + TICK_SLOT_WORD0, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&w[1], tick_words(h) + TICK_ERR_WORD, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *out = w[0];
    h->tick = w[0];
    if (w[1]) return fail(RSX_ERR_STATE, "step counter exhausted: a launch that would have wrapped it was refused on the device (a handle takes at most 2^32 - 1 fused steps)");
    return RSX_OK;
}

int rsx_task_placement_cache_stats(rsx_sim* h, int64_t out[2], void* stream) {
    RSX_ENTER_TASK(h);
    if (!out) return fail(RSX_ERR_ARG, "out is null");
    out[0] = out[1] = -1;   // -1: no cache on this handle, or the counters are off (RSX_PCACHE_STATS=1 before rsx_task_attach)
    if (!h->d_pcstats) return RSX_OK;
    HIP_TRY(hipMemcpyAsync(out, h->d_pcstats, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return RSX_OK;
}

int rsx_task_layout(rsx_sim* h, char* out, size_t n) {
    if (!h || !out || n == 0) return fail(RSX_ERR_ARG, "null argument");
    if (h->P.task == RSX_TASK_NONE) return fail(RSX_ERR_STATE, "no task attached (rsx_task_attach)");
    const char* name = h->epl ? "one-lane-per-env" : h->quad ? "four-lanes-per-env" : h->big ? "32-lanes-per-env-large-batch"
                     : h->L == 8 ? "8-lanes-per-env" : h->L == 16 ? "16-lanes-per-env" : h->L == 32 ? "32-lanes-per-env" : "64-lanes-per-env";
    std::snprintf(out, n, "%s", name);
    return RSX_OK;
}

int rsx_task_view_get(rsx_sim* h, rsx_task_view* out) {
    if (!h || !out) return fail(RSX_ERR_ARG, "null argument");
    if (h->P.task == RSX_TASK_NONE) return fail(RSX_ERR_STATE, "no task attached (rsx_task_attach)");
    const size_t B = (size_t)h->P.num_envs;
    out->task = h->P.task; out->obs_dim = h->P.obs_dim; out->act_dim = h->M.act_dim;
    out->info_dim = h->M.info_dim; out->max_episode_steps = h->P.max_steps;
    const size_t S = (size_t)h->P.row_stride;
    out->obs = h->d_obs; out->reward = h->d_aux + (size_t)ROW_REWARD * S;
    out->terminated = h->d_flags; out->truncated = h->d_flags + B;
    out->info = h->d_aux + (size_t)ROW_INFO * S; out->final_obs = h->d_final_obs;
    out->steps = (int32_t*)(h->d_aux + (size_t)ROW_STEPS * S); out->actions = h->d_actions;
    out->metrics = (int64_t*)h->d_metrics; out->row_stride = h->P.row_stride;
    return RSX_OK;
}

int rsx_task_reset(rsx_sim* h, void* stream) {
    RSX_ENTER_TASK(h);
    launch_task(h, nullptr, 1, MODE_RESET, (hipStream_t)stream);
    HIP_TRY(launch_status());
    h->task_ready = true;
    return RSX_OK;
}

int rsx_task_reset_to(rsx_sim* h, const double* ball, const double* blue, const double* yellow,
                      const uint8_t* env_mask, void* stream) {
    RSX_ENTER_TASK(h);
    if (int rc = rsx_reset(h, ball, blue, yellow, env_mask, stream)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t B = (size_t)h->P.num_envs;
    // the kernel takes the env mask through the third row of the flags array: `terminated` / `truncated` of the envs the mask leaves
    // alone stay what their last step made them (until round 6 the mask travelled through the `truncated` row, which was cleared
    // afterwards — for EVERY env: found by tests/test_gpu_api_fuzz.py)
    if (env_mask) HIP_TRY(hipMemcpyAsync(h->d_flags + 2 * B, env_mask, B, hipMemcpyHostToDevice, s));
    else HIP_TRY(hipMemsetAsync(h->d_flags + 2 * B, 1, B, s));
    launch_task(h, nullptr, 1, MODE_REFRESH, s);
    HIP_TRY(launch_status());
    HIP_TRY(hipStreamSynchronize(s));   // the host mask / placement arrays may be reused by the caller
    h->task_ready = true;
    return RSX_OK;
}

// The handle's step counter keys the per-step random draws and is one 32-bit word of the Philox counter: a handle that
// has taken 2^32 - 1 fused steps refuses further ones instead of silently replaying its random streams.
// Host-keyed handles (the default) check that here and bake the count into the launch — which is why they refuse to be
// captured: a replayed graph would step with one tick for ever.  Device-keyed handles (rsx_task_enable_capture) pass
// RSX_TICK_DEV instead: the kernels read, check and advance the counter themselves (rsx_kernels.hpp: step_tick).
static int step_prologue(rsx_sim* h, hipStream_t s, uint64_t n, int* flags) {
    *flags = 0;
    if (h->tick_dev) { *flags = RSX_TICK_DEV; return RSX_OK; }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) (void)hipGetLastError();   // (e.g. the legacy stream while another one captures: the launch reports it)
    else if (cs != hipStreamCaptureStatusNone)
        return fail(RSX_ERR_STATE, "this stream is being captured, and the handle's step counter (the key of its per-step random draws) is still a host-side "
                                   "launch argument: a replayed graph would repeat one random stream. Call rsx_task_enable_capture(h, stream) once, before the capture begins");
    if ((uint64_t)h->tick + n > 0xFFFFFFFFull)
        return fail(RSX_ERR_STATE, "step counter exhausted: a handle takes at most 2^32 - 1 fused steps (it keys the per-step random draws); attach a fresh handle with another seed");
    return RSX_OK;
}
// device-keyed handles: slots the launch did not cover (a grid without the placement helpers) follow slot 0
static void tick_resync(const rsx_sim* h, int mode, hipStream_t s) {
    if (h->tick_dev) tick_fill(h, step_grid(h, mode), h->tick_slots, 0u, 1, s);
}

int rsx_task_step(rsx_sim* h, const float* actions_dev, void* stream) {
    RSX_ENTER_TASK(h);
    RSX_NEED_RESET(h);
    int fl = 0;
    if (int rc = step_prologue(h, (hipStream_t)stream, 1, &fl)) return rc;
    h->P.tick_base = h->tick++;
    launch_task(h, actions_dev, 1 | fl, MODE_STEP, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return debug_finite(h, (hipStream_t)stream, "rsx_task_step");
}

int rsx_task_step_n(rsx_sim* h, int n, void* stream) {
    RSX_ENTER_TASK(h);
    RSX_NEED_RESET(h);
    if (n < 1) return fail(RSX_ERR_ARG, "n must be >= 1");
    int fl = 0;
    if (int rc = step_prologue(h, (hipStream_t)stream, (uint64_t)n, &fl)) return rc;
    for (int i = 0; i < n; ++i) { h->P.tick_base = h->tick++; launch_task(h, nullptr, 1 | fl, MODE_STEP, (hipStream_t)stream); }
    HIP_TRY(launch_status());
    return debug_finite(h, (hipStream_t)stream, "rsx_task_step_n");
}

int rsx_task_rollout(rsx_sim* h, int n, void* stream) {
    RSX_ENTER_TASK(h);
    RSX_NEED_RESET(h);
    if (n < 0 || n > RSX_N_STEPS_MASK) return fail(RSX_ERR_ARG, "n must be in 0 .. 2^30 - 1");  // 0 = load + store only (profiling)
    int fl = 0;
    if (int rc = step_prologue(h, (hipStream_t)stream, (uint64_t)n, &fl)) return rc;
    // (a device-keyed four-lane handle always takes the first form: all of its stepping launches then share one grid)
    if (h->quad && n >= 1 && (h->tick_dev || h->P.num_envs >= (h->P.task == RSX_TASK_SSL_SCRIMMAGE ? RSX_QUAD_ROLLOUT_MIN_ENVS : RSX_QUAD_ROLLOUT_MIN_ENVS_CROWDED))) {
        // 11v11 at large batches: n launches of the four-lanes-per-env kernel beat one launch of the 32-lane kernel
        // (262 144 envs, us per step: spread 182 vs 275, crowded 298 vs 340; crowded 131 072: 161 vs 164); same steps, same results
        for (int i = 0; i < n; ++i) { h->P.tick_base = h->tick++; launch_task(h, nullptr, 1 | fl, MODE_STEP, (hipStream_t)stream); }
        HIP_TRY(launch_status());
        return debug_finite(h, (hipStream_t)stream, "rsx_task_rollout");
    }
    h->P.tick_base = h->tick; h->tick += (uint32_t)n;
    launch_task(h, nullptr, n | fl, MODE_ROLLOUT, (hipStream_t)stream);
    tick_resync(h, MODE_ROLLOUT, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return debug_finite(h, (hipStream_t)stream, "rsx_task_rollout");
}

int rsx_task_lookahead(rsx_sim* h, const float* actions_dev, int n_candidates, int horizon, float gamma, float* returns_dev,
                       int32_t* steps_dev, uint8_t* flags_dev, float* last_obs_dev, void* stream) {
    RSX_ENTER(h);   // (not RSX_ENTER_TASK: nothing the handle owns changes, the host's copy of the state included)
    if (h->P.task == RSX_TASK_NONE) return fail(RSX_ERR_STATE, "no task attached (rsx_task_attach)");
    RSX_NEED_RESET(h);
    if (n_candidates < 1 || horizon < 1) return fail(RSX_ERR_ARG, "n_candidates and horizon must be >= 1");
    if (!actions_dev || !returns_dev || !steps_dev || !flags_dev) return fail(RSX_ERR_ARG, "actions_dev, returns_dev, steps_dev and flags_dev must not be null");
    if (!std::isfinite(gamma)) return fail(RSX_ERR_ARG, "gamma must be finite");
    if (h->L > 32) return fail(RSX_ERR_ARG, "rsx_task_lookahead has no 64-lanes-per-env kernels (unset RSX_LANES_PER_ENV)");
    if (lookahead_grid(h->L, h->P.num_envs, n_candidates) > 0x7FFFFFFFll)
        return fail(RSX_ERR_ARG, "num_envs x n_candidates exceeds the launch limit (2^31 - 1 workgroups): split the candidates over several calls");
    int fl = 0;
    if (int rc = step_prologue(h, (hipStream_t)stream, (uint64_t)horizon, &fl)) return rc;   // capture of a host-keyed handle, counter limit
    Params P = h->P;
    P.tick_base = h->tick;   // the tick the next step would take; not advanced
    launch_task_lookahead(P, h->L, h->NR, h->d_state, h->d_aux, h->tick_dev ? tick_words(h) + TICK_SLOT_WORD0 : nullptr, h->d_phys,
                          actions_dev, n_candidates, horizon, gamma, returns_dev, steps_dev, flags_dev, last_obs_dev, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_check_finite(rsx_sim* h, int64_t* n_bad, void* stream) {
    RSX_ENTER(h);
    if (!n_bad) return fail(RSX_ERR_ARG, "n_bad is null");
    return check_finite_impl(h, n_bad, (hipStream_t)stream);
}

}  // extern "C" (reopened below)

// ---- task checkpoint: everything a fused run needs to continue bit-identically ----
namespace {
struct CkptHeader {
    uint64_t magic;            // "RSXCKPT2"
    int32_t abi, kind, field_rows, task, n_blue, n_yellow, num_envs, state_rows, aux_rows, obs_dim;
    int32_t field_type, time_step_ms, max_steps, model;   // model: RSX_PHYSICS_MODEL of the saving library
    uint32_t key0, key1, env_id_base, tick;
    uint64_t state_bytes, aux_bytes, obs_bytes, flag_bytes;
    int64_t metrics[RSX_METRICS];
};
constexpr uint64_t CKPT_MAGIC = 0x3254504B43585352ull;   // "RSXCKPT2", little endian
// model word of a physics-enabled handle's blob: a section follows the others — the physics header (ranges), the parameter rows
// and the coefficient rows (dense, like the rest); a blob of either kind is refused by a handle of the other
constexpr int32_t CKPT_MODEL_PHYS = 1 << 16;
size_t ckpt_phys_bytes(const CkptHeader& k) {
    return (k.model & CKPT_MODEL_PHYS) ? sizeof(PhysHeader) + (size_t)(NPHYS + NCOEF) * (size_t)k.num_envs * sizeof(float) : 0;
}
CkptHeader ckpt_header(const rsx_sim* h) {
    CkptHeader k{};
    const size_t B = (size_t)h->P.num_envs;
    k.magic = CKPT_MAGIC; k.abi = RSX_ABI_VERSION; k.kind = h->P.kind; k.field_rows = h->M.rs; k.task = h->P.task;
    k.n_blue = h->P.n_blue; k.n_yellow = h->P.n_yellow; k.num_envs = h->P.num_envs;
    k.state_rows = h->P.state_dim + X_ROWS; k.aux_rows = aux_rows(h->P.n_robots); k.obs_dim = h->P.obs_dim;
    k.field_type = h->field_type; k.time_step_ms = h->time_step_ms; k.max_steps = h->P.max_steps; k.model = RSX_PHYSICS_MODEL | (h->d_phys ? CKPT_MODEL_PHYS : 0);
    k.key0 = h->P.key0; k.key1 = h->P.key1; k.env_id_base = h->P.env_id_base; k.tick = h->tick;
    k.state_bytes = (uint64_t)k.state_rows * B * sizeof(float);
    k.aux_bytes = (uint64_t)k.aux_rows * B * sizeof(float);
    k.obs_bytes = (uint64_t)B * k.obs_dim * sizeof(float);
    k.flag_bytes = 2 * B;
    return k;
}
size_t ckpt_size(const CkptHeader& k) { return sizeof(CkptHeader) + k.state_bytes + k.aux_bytes + 2 * k.obs_bytes + k.flag_bytes + ckpt_phys_bytes(k); }
}  // namespace

extern "C" {

int rsx_task_checkpoint_size(rsx_sim* h, size_t* bytes) {
    if (!h || !bytes) return fail(RSX_ERR_ARG, "null argument");
    if (h->P.task == RSX_TASK_NONE) return fail(RSX_ERR_STATE, "no task attached (rsx_task_attach)");
    *bytes = ckpt_size(ckpt_header(h));
    return RSX_OK;
}

int rsx_task_checkpoint_save(rsx_sim* h, void* blob, size_t bytes, void* stream) {
    RSX_ENTER_TASK(h);
    if (!blob) return fail(RSX_ERR_ARG, "blob is null");
    CkptHeader k = ckpt_header(h);
    if (bytes < ckpt_size(k)) return fail(RSX_ERR_ARG, "blob is smaller than rsx_task_checkpoint_size");
    hipStream_t s = (hipStream_t)stream;
    rsx_launch(fold_metrics_kernel, dim3(1), dim3(64), 0, s, h->d_metrics, h->d_mslots);
    HIP_TRY(launch_status());
    char* p = (char*)blob + sizeof(CkptHeader);
    // (the blob's rows are dense — B floats — whatever the row pad of this handle: it restores into any layout)
    const size_t rowb = (size_t)h->P.num_envs * sizeof(float), pitch = (size_t)h->P.row_stride * sizeof(float);
    HIP_TRY(hipMemcpy2DAsync(p, rowb, h->d_state, pitch, rowb, (size_t)k.state_rows, hipMemcpyDeviceToHost, s)); p += k.state_bytes;
    HIP_TRY(hipMemcpy2DAsync(p, rowb, h->d_aux, pitch, rowb, (size_t)k.aux_rows, hipMemcpyDeviceToHost, s)); p += k.aux_bytes;
    HIP_TRY(hipMemcpyAsync(p, h->d_obs, k.obs_bytes, hipMemcpyDeviceToHost, s)); p += k.obs_bytes;
    HIP_TRY(hipMemcpyAsync(p, h->d_final_obs, k.obs_bytes, hipMemcpyDeviceToHost, s)); p += k.obs_bytes;
    HIP_TRY(hipMemcpyAsync(p, h->d_flags, k.flag_bytes, hipMemcpyDeviceToHost, s));
    if (h->d_phys) {
        p += k.flag_bytes;
        HIP_TRY(hipMemcpyAsync(p, h->d_phys, sizeof(PhysHeader), hipMemcpyDeviceToHost, s)); p += sizeof(PhysHeader);
        HIP_TRY(hipMemcpy2DAsync(p, rowb, phys_raw(h->d_phys), pitch, rowb, (size_t)(NPHYS + NCOEF), hipMemcpyDeviceToHost, s));   // raw rows, then the coefficient rows
    }
    HIP_TRY(hipMemcpyAsync(k.metrics, h->d_metrics, sizeof(k.metrics), hipMemcpyDeviceToHost, s));
    if (h->tick_dev)   // device-keyed handle: the step counter is slot 0 of the per-workgroup slots (all equal between launches)
        HIP_TRY(hipMemcpyAsync(&k.tick, tick_words(h) + TICK_SLOT_WORD0, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h->tick_dev) h->tick = k.tick;
    std::memcpy(blob, &k, sizeof(k));
    if (h->P.task == RSX_TASK_VSS_V0) {
        // The task scalar of VSS-v0 (previous ball potential, vss_gym.py:256-283) is a function of the ball position
        // the next step starts from; the one-lane-per-env kernel recomputes it instead of keeping the row up to date.
        // The blob always carries the value, so that it restores into either kernel layout.  Same float expression
        // as the kernels' (this file is built with -ffp-contract=off; sqrtf is correctly rounded on both sides).
        const size_t B = (size_t)h->P.num_envs;
        const float* st = reinterpret_cast<const float*>((const char*)blob + sizeof(CkptHeader));
        float* aux = reinterpret_cast<float*>((char*)blob + sizeof(CkptHeader) + k.state_bytes);
        for (size_t e = 0; e < B; ++e) {
            const float bx = st[e], by = st[B + e];
            const float dx_d = (h->P.hl_goal + bx) * 100.0f, dx_a = (h->P.hl_goal - bx) * 100.0f, dy = by * 100.0f;
            const float dy2 = 2.0f * (dy * dy);
            const float dist_1 = -std::sqrt(dx_a * dx_a + dy2), dist_2 = std::sqrt(dx_d * dx_d + dy2);
            aux[(size_t)ROW_PREV_POT * B + e] = ((dist_1 + dist_2) * h->P.inv_len_cm - 1.0f) * 0.5f;
        }
    }
    return RSX_OK;
}

int rsx_task_checkpoint_load(rsx_sim* h, const void* blob, size_t bytes, void* stream) {
    RSX_ENTER_TASK(h);
    if (!blob || bytes < sizeof(CkptHeader)) return fail(RSX_ERR_ARG, "blob is null or truncated");
    CkptHeader k;
    std::memcpy(&k, blob, sizeof(k));
    CkptHeader want = ckpt_header(h);
    if (k.magic != CKPT_MAGIC || k.abi != want.abi) return fail(RSX_ERR_ARG, "not a checkpoint of this library version");
    if ((k.model & CKPT_MODEL_PHYS) != (want.model & CKPT_MODEL_PHYS))
        return fail(RSX_ERR_ARG, "the checkpoint was taken from a handle with per-env physics on / off and this one has it off / on (rsx_physics_enable)");
    if (k.model != want.model) return fail(RSX_ERR_ARG, "the checkpoint was taken under another version of the physics model (RSX_PHYSICS_MODEL)");
    if (k.kind != want.kind || k.task != want.task || k.n_blue != want.n_blue || k.n_yellow != want.n_yellow ||
        k.num_envs != want.num_envs || k.state_rows != want.state_rows || k.aux_rows != want.aux_rows || k.obs_dim != want.obs_dim)
        return fail(RSX_ERR_ARG, "the checkpoint was taken from a different configuration (simulator kind, team sizes, batch or task)");
    if (k.field_type != want.field_type || k.time_step_ms != want.time_step_ms || k.field_rows != want.field_rows)
        return fail(RSX_ERR_ARG, "the checkpoint was taken with another field type or time step");
    if (k.max_steps != want.max_steps)
        return fail(RSX_ERR_ARG, "the checkpoint was taken with another max_episode_steps (TimeLimit)");
    if (k.key0 != want.key0 || k.key1 != want.key1 || k.env_id_base != want.env_id_base)
        return fail(RSX_ERR_ARG, "the checkpoint was taken with another seed or env_id_base: attach the task with the same ones");
    // the section sizes follow from the configuration checked above; they are used for pointer arithmetic and as copy lengths below,
    // so a header that disagrees (a damaged file) is refused instead of being trusted
    if (k.state_bytes != want.state_bytes || k.aux_bytes != want.aux_bytes || k.obs_bytes != want.obs_bytes || k.flag_bytes != want.flag_bytes)
        return fail(RSX_ERR_ARG, "the checkpoint header is damaged (section sizes do not match its configuration)");
    if (bytes < ckpt_size(k)) return fail(RSX_ERR_ARG, "blob is truncated");
    hipStream_t s = (hipStream_t)stream;
    const char* p = (const char*)blob + sizeof(CkptHeader);
    h->host_state_valid = false;
    const size_t rowb = (size_t)h->P.num_envs * sizeof(float), pitch = (size_t)h->P.row_stride * sizeof(float);
    HIP_TRY(hipMemcpy2DAsync(h->d_state, pitch, p, rowb, rowb, (size_t)k.state_rows, hipMemcpyHostToDevice, s)); p += k.state_bytes;
    HIP_TRY(hipMemcpy2DAsync(h->d_aux, pitch, p, rowb, rowb, (size_t)k.aux_rows, hipMemcpyHostToDevice, s)); p += k.aux_bytes;
    HIP_TRY(hipMemcpyAsync(h->d_obs, p, k.obs_bytes, hipMemcpyHostToDevice, s)); p += k.obs_bytes;
    HIP_TRY(hipMemcpyAsync(h->d_final_obs, p, k.obs_bytes, hipMemcpyHostToDevice, s)); p += k.obs_bytes;
    HIP_TRY(hipMemcpyAsync(h->d_flags, p, k.flag_bytes, hipMemcpyHostToDevice, s));
    if (h->d_phys) {   // ranges and mask of the blob, this handle's error word
        p += k.flag_bytes;
        PhysHeader hd;
        std::memcpy(&hd, p, sizeof(hd)); p += sizeof(PhysHeader);
        if (hd.kind != h->P.kind || hd.ts_ms != h->time_step_ms) return fail(RSX_ERR_ARG, "the checkpoint's physics section is damaged");
        launch_phys_ranges(h->d_phys, hd.lo, hd.hi, hd.mask, s);
        HIP_TRY(launch_status());
        HIP_TRY(hipMemcpy2DAsync(phys_raw(h->d_phys), pitch, p, rowb, rowb, (size_t)(NPHYS + NCOEF), hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemsetAsync(h->d_mslots, 0, (size_t)MSLOTS * RSX_METRICS * sizeof(unsigned long long), s));
    HIP_TRY(hipMemcpyAsync(h->d_metrics, k.metrics, sizeof(k.metrics), hipMemcpyHostToDevice, s));
    if (h->tick_dev) {   // device-keyed handle: every slot takes the blob's step counter; a refused-launch mark is cleared with it
        tick_fill(h, 0, h->tick_slots_alloc, k.tick, 0, s);
        HIP_TRY(launch_status());
        HIP_TRY(hipMemsetAsync(tick_words(h) + TICK_ERR_WORD, 0, sizeof(uint32_t), s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    h->tick = k.tick;
    h->task_ready = true;
    return RSX_OK;
}

}  // extern "C"

extern "C" {
int rsx_metrics_fold(rsx_sim* h, void* stream) {
    RSX_ENTER_TASK(h);
    rsx_launch(fold_metrics_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, h->d_metrics, h->d_mslots);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_read_metrics(rsx_sim* h, int64_t out[RSX_METRICS], void* stream) {
    RSX_ENTER_TASK(h);
    if (!out) return fail(RSX_ERR_ARG, "out is null");
    hipStream_t s = (hipStream_t)stream;
    rsx_launch(fold_metrics_kernel, dim3(1), dim3(64), 0, s, h->d_metrics, h->d_mslots);
    HIP_TRY(launch_status());
    HIP_TRY(hipMemcpyAsync(out, h->d_metrics, RSX_METRICS * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    uint32_t refused = 0;
    if (h->tick_dev) HIP_TRY(hipMemcpyAsync(&refused, tick_words(h) + TICK_ERR_WORD, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (refused) return fail(RSX_ERR_STATE, "step counter exhausted: stepping launches of this device-keyed handle were refused on the device (out[] is valid; a handle takes at most 2^32 - 1 fused steps)");
    return RSX_OK;
}

}  // extern "C"

// ---- per-env physics parameters (rsx.h: rsx_physics_*; kernels and block layout: rsx_phys.hip, rsx_phys.hpp) ----
namespace {
int check_phys_set(int kind, const float* raw) {
    for (int p = 0; p < NPHYS; ++p)
        if (!phys_valid(kind, p, raw[p])) return fail(RSX_ERR_ARG, "physics parameter " + std::to_string(p) + " out of range (rsx.h: rsx_physics_*)");
    return RSX_OK;
}
}  // namespace

extern "C" {

int rsx_physics_defaults(int kind, float out[RSX_PHYS_PARAMS]) {
    if (kind != RSX_KIND_VSS && kind != RSX_KIND_SSL) return fail(RSX_ERR_ARG, "kind must be RSX_KIND_VSS or RSX_KIND_SSL");
    if (!out) return fail(RSX_ERR_ARG, "out is null");
    for (int p = 0; p < NPHYS; ++p) out[p] = (float)phys_default(kind, p);
    return RSX_OK;
}

int rsx_physics_derive(int kind, int time_step_ms, const float raw[RSX_PHYS_PARAMS], float coef[RSX_PHYS_COEFS]) {
    if (kind != RSX_KIND_VSS && kind != RSX_KIND_SSL) return fail(RSX_ERR_ARG, "kind must be RSX_KIND_VSS or RSX_KIND_SSL");
    if (!raw || !coef || time_step_ms < 0) return fail(RSX_ERR_ARG, "null argument or negative time step");
    if (int rc = check_phys_set(kind, raw)) return rc;
    derive_coefs(kind, time_step_ms, raw, coef);
    return RSX_OK;
}

int rsx_physics_enable(rsx_sim* h, void* stream) {
    RSX_ENTER(h);
    if (h->d_phys) return RSX_OK;
    if (h->L > 32) return fail(RSX_ERR_ARG, "per-env physics runs with up to 32 lanes per env (unset RSX_LANES_PER_ENV=64)");
    if (h->tick_dev) return fail(RSX_ERR_STATE, "call rsx_physics_enable before rsx_task_enable_capture");
    hipStream_t s = (hipStream_t)stream;
    const size_t S = (size_t)h->P.row_stride;
    HIP_TRY(hipMalloc((void**)&h->d_phys, phys_block_bytes(S)));
    HIP_TRY(hipMemsetAsync(h->d_phys, 0, phys_block_bytes(S), s));
    PhysHeader hd{};
    hd.kind = h->P.kind; hd.ts_ms = h->time_step_ms;
    HIP_TRY(hipMemcpyAsync(h->d_phys, &hd, sizeof(hd), hipMemcpyHostToDevice, s));
    launch_phys_init(h->d_phys, h->P.num_envs, (int)S, h->P.kind, h->time_step_ms, s);
    HIP_TRY(launch_status());
    HIP_TRY(hipStreamSynchronize(s));   // (the header travels from the stack)
    if (h->P.task != RSX_TASK_NONE) {   // attached already: the layout of a physics-enabled handle
        h->epl = h->big = h->quad = false;
        h->tick_slots = step_grid(h, MODE_STEP);
    }
    return RSX_OK;
}

int rsx_physics_set(rsx_sim* h, const float* values, int on_device, const uint8_t* env_mask, void* stream) {
    RSX_ENTER(h);
    if (!h->d_phys) return fail(RSX_ERR_STATE, "per-env physics is off (rsx_physics_enable)");
    if (!values) return fail(RSX_ERR_ARG, "values is null");
    hipStream_t s = (hipStream_t)stream;
    const int B = h->P.num_envs;
    const size_t S = (size_t)h->P.row_stride;
    h->host_state_valid = false;
    if (on_device) {
        launch_phys_set(h->d_phys, values, env_mask, B, (int)S, B, s);
        HIP_TRY(launch_status());
        return RSX_OK;
    }
    // host values: checked here (NaN = keep), then staged and written by the same kernel
    for (int e = 0; e < B; ++e) {
        if (env_mask && !env_mask[e]) continue;
        for (int p = 0; p < NPHYS; ++p) {
            const float v = values[(size_t)p * B + e];
            if (v == v && !phys_valid(h->P.kind, p, v))
                return fail(RSX_ERR_ARG, "physics parameter " + std::to_string(p) + " of env " + std::to_string(e) + " out of range (rsx.h: rsx_physics_*)");
        }
    }
    float* const stage = phys_stage(h->d_phys, S);
    uint8_t* const smask = phys_stage_mask(h->d_phys, S);
    HIP_TRY(hipMemcpyAsync(stage, values, (size_t)NPHYS * B * sizeof(float), hipMemcpyHostToDevice, s));
    if (env_mask) HIP_TRY(hipMemcpyAsync(smask, env_mask, (size_t)B, hipMemcpyHostToDevice, s));
    launch_phys_set(h->d_phys, stage, env_mask ? smask : nullptr, B, (int)S, B, s);
    HIP_TRY(launch_status());
    HIP_TRY(hipStreamSynchronize(s));   // the caller's arrays may go away on return
    return RSX_OK;
}

int rsx_physics_get(rsx_sim* h, int which, float* out, void* stream) {
    RSX_ENTER(h);
    if (!h->d_phys) return fail(RSX_ERR_STATE, "per-env physics is off (rsx_physics_enable)");
    if (!out || (which != RSX_PHYS_RAW && which != RSX_PHYS_COEF)) return fail(RSX_ERR_ARG, "out is null or `which` unknown");
    hipStream_t s = (hipStream_t)stream;
    const size_t S = (size_t)h->P.row_stride, rowb = (size_t)h->P.num_envs * sizeof(float);
    const float* src = which == RSX_PHYS_RAW ? phys_raw(h->d_phys) : phys_coef(h->d_phys, S);
    HIP_TRY(hipMemcpy2DAsync(out, rowb, src, S * sizeof(float), rowb, (size_t)(which == RSX_PHYS_RAW ? NPHYS : NCOEF), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return RSX_OK;
}

int rsx_physics_randomize(rsx_sim* h, const float* lo, const float* hi, uint32_t param_mask, void* stream) {
    RSX_ENTER(h);
    if (!h->d_phys) return fail(RSX_ERR_STATE, "per-env physics is off (rsx_physics_enable)");
    if (param_mask >> NPHYS) return fail(RSX_ERR_ARG, "param_mask names a parameter that does not exist");
    if (param_mask && (!lo || !hi)) return fail(RSX_ERR_ARG, "lo / hi are null");
    for (int p = 0; p < NPHYS; ++p) {
        if (!((param_mask >> p) & 1u)) continue;
        if (!phys_valid(h->P.kind, p, lo[p]) || !phys_valid(h->P.kind, p, hi[p]) || !(lo[p] <= hi[p]))
            return fail(RSX_ERR_ARG, "randomisation range of physics parameter " + std::to_string(p) + " is invalid (lo <= hi, both valid values)");
    }
    launch_phys_ranges(h->d_phys, param_mask ? lo : nullptr, param_mask ? hi : nullptr, param_mask, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_physics_errors(rsx_sim* h, int64_t* out, void* stream) {
    RSX_ENTER(h);
    if (!h->d_phys) return fail(RSX_ERR_STATE, "per-env physics is off (rsx_physics_enable)");
    if (!out) return fail(RSX_ERR_ARG, "out is null");
    hipStream_t s = (hipStream_t)stream;
    uint32_t* const w = &reinterpret_cast<PhysHeader*>(h->d_phys)->err;
    uint32_t v = 0;
    HIP_TRY(hipMemcpyAsync(&v, w, sizeof(v), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(w, 0, sizeof(uint32_t), s));
    HIP_TRY(hipStreamSynchronize(s));
    *out = (int64_t)v;
    return RSX_OK;
}

// ---- trace evaluation (rsx.h: rsx_trace_*; kernel: rsx_sysid.hip) ----
int rsx_trace_load(rsx_sim* h, const double* frames, const double* cmds, int n_frames, const int32_t* anchors, int n_anchors,
                   void* stream) {
    RSX_ENTER(h);
    if (!h->d_phys) return fail(RSX_ERR_STATE, "trace evaluation needs per-env physics (rsx_physics_enable)");
    if (h->P.task != RSX_TASK_NONE) return fail(RSX_ERR_STATE, "trace evaluation runs on a raw handle: a task is attached");
    if (!frames || !cmds || !anchors) return fail(RSX_ERR_ARG, "null argument");
    if (n_frames < 2 || n_anchors < 1) return fail(RSX_ERR_ARG, "a trace needs n_frames >= 2 and n_anchors >= 1");
    if (h->P.num_envs % n_anchors != 0) return fail(RSX_ERR_ARG, "num_envs must be a multiple of n_anchors");
    const int rows = h->P.state_dim + X_ROWS, NC = h->P.n_robots * h->M.cmd_dim;
    const size_t F = (size_t)n_frames, T = F - 1;
    if ((size_t)rows * F * sizeof(float) >= ((size_t)1 << 32) || (size_t)NC * T * sizeof(float) >= ((size_t)1 << 32))
        return fail(RSX_ERR_ARG, "trace too long: its arrays would reach 4 GB");
    int amax = 0;
    for (int a = 0; a < n_anchors; ++a) {
        if (anchors[a] < 0 || anchors[a] > n_frames - 2) return fail(RSX_ERR_ARG, "anchor " + std::to_string(a) + " outside [0, n_frames - 2]");
        amax = std::max(amax, (int)anchors[a]);
    }
    const size_t fbytes = align_up((size_t)rows * F * sizeof(float)), cbytes = align_up((size_t)NC * T * sizeof(float));
    std::vector<char> host(fbytes + cbytes + (size_t)n_anchors * sizeof(int32_t), 0);
    float* const hf = reinterpret_cast<float*>(host.data());
    float* const hc = reinterpret_cast<float*>(host.data() + fbytes);
    for (size_t f = 0; f < F; ++f)
        for (int r = 0; r < rows; ++r) {
            const double v = frames[f * rows + r];
            if (!std::isfinite(v)) return fail(RSX_ERR_ARG, "non-finite value in frame " + std::to_string(f));
            hf[(size_t)r * F + f] = (float)v;
        }
    for (size_t t = 0; t < T; ++t)
        for (int j = 0; j < NC; ++j) {
            const double v = cmds[t * NC + j];
            if (!std::isfinite(v)) return fail(RSX_ERR_ARG, "non-finite value in the commands of step " + std::to_string(t));
            hc[(size_t)j * T + t] = (float)v;
        }
    std::memcpy(host.data() + fbytes + cbytes, anchors, (size_t)n_anchors * sizeof(int32_t));
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipStreamSynchronize(s));   // a trace loaded before may still be read by a launch in flight
    if (h->d_trace) { HIP_TRY(hipFree(h->d_trace)); h->d_trace = nullptr; h->trace_frames = 0; }
    HIP_TRY(hipMalloc((void**)&h->d_trace, host.size()));
    HIP_TRY(hipMemcpyAsync(h->d_trace, host.data(), host.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    h->trace_frames = n_frames; h->trace_anchors = n_anchors; h->trace_anchor_max = amax;
    h->trace_cmds_off = fbytes; h->trace_anchors_off = fbytes + cbytes;
    return RSX_OK;
}

int rsx_trace_eval(rsx_sim* h, int horizon, float* loss_dev, void* stream) {
    RSX_ENTER(h);
    if (!h->d_phys) return fail(RSX_ERR_STATE, "trace evaluation needs per-env physics (rsx_physics_enable)");
    if (h->P.task != RSX_TASK_NONE) return fail(RSX_ERR_STATE, "trace evaluation runs on a raw handle: a task is attached");
    if (!h->d_trace) return fail(RSX_ERR_STATE, "no trace loaded (rsx_trace_load)");
    if (!loss_dev) return fail(RSX_ERR_ARG, "loss_dev is null");
    if (horizon < 1 || (int64_t)h->trace_anchor_max + horizon > (int64_t)h->trace_frames - 1)
        return fail(RSX_ERR_ARG, "horizon must be >= 1 and every anchor + horizon <= n_frames - 1");
    h->host_state_valid = false;
    const char* const base = reinterpret_cast<const char*>(h->d_trace);
    launch_trace_eval(h->P, h->L, h->NR, h->d_phys, h->d_state, loss_dev, h->d_trace, reinterpret_cast<const float*>(base + h->trace_cmds_off),
                      reinterpret_cast<const int32_t*>(base + h->trace_anchors_off), h->trace_frames, h->trace_anchors, horizon, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return debug_finite(h, (hipStream_t)stream, "rsx_trace_eval");
}

// ---- batched rgb frames (rsx.h: rsx_render_*; field image and kernel: rsx_render.hip) ----
int rsx_render_view_reference(int kind, rsx_render_view* out) {
    if (!out || (kind != RSX_KIND_VSS && kind != RSX_KIND_SSL)) return fail(RSX_ERR_ARG, "out is null or `kind` unknown");
    // Render/raster.py: VSS_VIEW / SSL_VIEW (raster.py is the specification and stays as it is, so the values stand here once more;
    // tests/test_render_batch.py::test_views holds the two, and Render.reference_view, together)
    if (kind == RSX_KIND_VSS) *out = rsx_render_view{1.5, 1.3, 0.1, 0.2, 0.15, 0.7, 0.4, 0.1, 500.0, 0.04, 0.0215, 1};
    else *out = rsx_render_view{9.0, 6.0, 0.35, 1.0, 1.0, 2.0, 1.0, 0.18, 100.0, 0.09, 0.0215, 0};
    return RSX_OK;
}

int rsx_render_size(const rsx_render_view* v, int* width, int* height) {
    if (!width || !height) return fail(RSX_ERR_ARG, "null argument");
    if (const char* msg = render_check_view(v, width, height)) return fail(RSX_ERR_ARG, msg);
    return RSX_OK;
}

int rsx_render_field(const rsx_render_view* v, uint8_t* out_hwc) {
    int W = 0, H = 0;
    if (const char* msg = render_check_view(v, &W, &H)) return fail(RSX_ERR_ARG, msg);
    if (!out_hwc) return fail(RSX_ERR_ARG, "out_hwc is null");
    render_field_host(*v, W, H, out_hwc);
    return RSX_OK;
}

// views a handle may hold (none is freed before rsx_destroy: see rsx_sim::render_views)
#ifndef RSX_RENDER_MAX_VIEWS
#define RSX_RENDER_MAX_VIEWS 16
#endif

int rsx_render_open(rsx_sim* h, const rsx_render_view* v, void* stream) {
    RSX_ENTER(h);
    int W = 0, H = 0;
    if (const char* msg = render_check_view(v, &W, &H)) return fail(RSX_ERR_ARG, msg);
    for (size_t i = 0; i < h->render_views.size(); ++i) {   // a view the handle already holds: selected, nothing else happens
        const rsx_render_view& o = h->render_views[i].view;
        if (o.length == v->length && o.width == v->width && o.margin == v->margin && o.circle == v->circle && o.pen_len == v->pen_len &&
            o.pen_wid == v->pen_wid && o.goal_wid == v->goal_wid && o.goal_dep == v->goal_dep && o.scale == v->scale &&
            o.robot == v->robot && o.ball == v->ball && o.square == v->square) {
            h->render_cur = (int)i;
            return RSX_OK;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    {   // a new view allocates, uploads and synchronises: not inside a capture
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs) != hipSuccess) (void)hipGetLastError();
        else if (cs != hipStreamCaptureStatusNone) return fail(RSX_ERR_STATE, "rsx_render_open of a new view cannot be captured: open it before the capture");
    }
    if ((int)h->render_views.size() >= RSX_RENDER_MAX_VIEWS)
        return fail(RSX_ERR_STATE, "the handle holds " + std::to_string(RSX_RENDER_MAX_VIEWS) + " render views already (views live until rsx_destroy: captured launches may read them)");
    const size_t HW = (size_t)W * (size_t)H, fb = 3 * HW, tpl = align_up(fb);
    std::vector<uint8_t> host(2 * tpl, 0);
    uint8_t* const hwc = host.data();
    uint8_t* const chw = hwc + tpl;
    render_field_host(*v, W, H, hwc);
    for (size_t p = 0; p < HW; ++p)
        for (size_t c = 0; c < 3; ++c) chw[c * HW + p] = hwc[3 * p + c];
    if (!h->d_render_err) {
        HIP_TRY(hipMalloc((void**)&h->d_render_err, 256));
        HIP_TRY(hipMemsetAsync(h->d_render_err, 0, 256, s));
    }
    rsx_sim::RenderSlot rv{*v, render_geom(*v, W, H), nullptr, tpl};
    HIP_TRY(hipMalloc((void**)&rv.tpl, host.size()));
    hipError_t e = hipMemcpyAsync(rv.tpl, host.data(), host.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipFree(rv.tpl); return fail(RSX_ERR_HIP, std::string("rsx_render_open upload: ") + hipGetErrorString(e)); }
    h->render_views.push_back(rv);
    h->render_cur = (int)h->render_views.size() - 1;
    return RSX_OK;
}

int rsx_render(rsx_sim* h, const int32_t* env_ids_dev, int n, int channels_first, uint8_t* out_dev, void* stream) {
    RSX_ENTER(h);
    if (h->render_cur < 0) return fail(RSX_ERR_STATE, "no render view (rsx_render_open)");
    if (!out_dev || ((uintptr_t)out_dev & 15u)) return fail(RSX_ERR_ARG, "out_dev must be a 16-byte aligned device pointer");
    if (n < 1 || (!env_ids_dev && n > h->P.num_envs)) return fail(RSX_ERR_ARG, "n must be >= 1, and <= num_envs without env_ids_dev");
    const rsx_sim::RenderSlot& rv = h->render_views[(size_t)h->render_cur];
    launch_render(rv.geom, h->d_state, h->P.num_envs, h->P.row_stride, h->P.kind, h->P.n_blue, h->P.n_yellow,
                  rv.tpl + (channels_first ? rv.tpl_bytes : 0), h->d_render_err, env_ids_dev, n, channels_first != 0, out_dev, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_render_errors(rsx_sim* h, int64_t* out, void* stream) {
    RSX_ENTER(h);
    if (!h->d_render_err) return fail(RSX_ERR_STATE, "no render view (rsx_render_open)");
    if (!out) return fail(RSX_ERR_ARG, "out is null");
    hipStream_t s = (hipStream_t)stream;
    uint32_t v = 0;
    HIP_TRY(hipMemcpyAsync(&v, h->d_render_err, sizeof(v), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(h->d_render_err, 0, sizeof(uint32_t), s));
    HIP_TRY(hipStreamSynchronize(s));
    *out = (int64_t)v;
    return RSX_OK;
}

// ---- transfer of running episodes between envs and handles ----
// the count of skipped pairs lives in a spare word of the task arena's metrics block (metrics[8] | ... | step-counter slots from
// TICK_SLOT_WORD0), zeroed by rsx_task_attach / rsx_task_reseed: a cross-handle transfer allocates nothing
constexpr int XFER_ERR_WORD = 20;
static_assert(XFER_ERR_WORD >= 2 * RSX_METRICS && XFER_ERR_WORD != TICK_ERR_WORD && XFER_ERR_WORD < TICK_SLOT_WORD0, "spare word of the metrics block");

static XferSide xfer_side_of(const rsx_sim* h) {
    return XferSide{h->d_state, h->d_aux, h->d_phys ? phys_raw(h->d_phys) : nullptr, h->d_obs, h->d_final_obs, h->d_flags,
                    h->P.row_stride, h->P.num_envs};
}

int rsx_task_transfer(rsx_sim* dst, rsx_sim* src, const int32_t* dst_ids_dev, const int32_t* src_ids_dev, int n, void* stream) {
    if (!src) return fail(RSX_ERR_ARG, "null handle");
    RSX_ENTER_TASK(dst);
    if (src->P.task == RSX_TASK_NONE) return fail(RSX_ERR_STATE, "no task attached to the source (rsx_task_attach)");
    if (!dst->task_ready || !src->task_ready)
        return fail(RSX_ERR_STATE, "rsx_task_reset / rsx_task_reset_to must come before rsx_task_transfer, on both handles");
    if (src->device != dst->device) return fail(RSX_ERR_ARG, "the handles live on different devices");
    const Params &D = dst->P, &S = src->P;
    if (D.kind != S.kind || D.task != S.task || D.n_blue != S.n_blue || D.n_yellow != S.n_yellow)
        return fail(RSX_ERR_ARG, "the handles differ in simulator kind, task or team sizes");
    if (dst->field_type != src->field_type || dst->time_step_ms != src->time_step_ms)
        return fail(RSX_ERR_ARG, "the handles differ in field type or time step");
    if (D.max_steps != S.max_steps) return fail(RSX_ERR_ARG, "the handles differ in max_episode_steps (TimeLimit)");
    if ((dst->d_phys != nullptr) != (src->d_phys != nullptr))
        return fail(RSX_ERR_ARG, "per-env physics is enabled on one handle only (rsx_physics_enable)");
    if (n < 0) return fail(RSX_ERR_ARG, "n must be >= 0");
    if ((!dst_ids_dev && n > D.num_envs) || (!src_ids_dev && n > S.num_envs))
        return fail(RSX_ERR_ARG, "n exceeds num_envs of a side without an id array (NULL = envs 0..n-1)");
    if (n == 0) return RSX_OK;
    hipStream_t s = (hipStream_t)stream;
    const int SR = D.state_dim + X_ROWS, AR = aux_rows(D.n_robots), PR = dst->d_phys ? NPHYS + NCOEF : 0, OD = D.obs_dim;
    const int pot_row = D.task == RSX_TASK_VSS_V0 ? SR + ROW_PREV_POT : -1;
    uint32_t* const err = tick_words(dst) + XFER_ERR_WORD;
    // (the placement cache of either handle needs no invalidation: an entry is tagged with the episode id it was made for and is a
    // pure function of (seed, global env id, episode) — a tag that no longer matches takes the inline path, one that matches by
    // coincidence holds the right placement)
    if (dst != src) {
        launch_transfer(XFER_DIRECT, xfer_side_of(dst), xfer_side_of(src), D.num_envs, S.num_envs, dst_ids_dev, src_ids_dev, n, err,
                        SR, AR, PR, OD, pot_row, D.hl_goal, D.inv_len_cm, s);
        HIP_TRY(launch_status());
        return RSX_OK;
    }
    // same handle: every read before every write — gather the n records into the staging buffer, then scatter them
    rsx_sim* const h = dst;
    if (n > h->xfer_cap) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs) != hipSuccess) (void)hipGetLastError();
        else if (cs != hipStreamCaptureStatusNone)
            return fail(RSX_ERR_STATE, "a same-handle rsx_task_transfer whose staging buffer has to grow cannot be captured: make one eager call with n = " +
                                       std::to_string(n) + " (or more) before the capture");
        HIP_TRY(hipStreamSynchronize(s));
        char* p = nullptr;
        const size_t cap = (size_t)n;
        const size_t bytes = 3 * align_up((size_t)std::max(SR, std::max(AR, NPHYS + NCOEF)) * cap * sizeof(float)) +
                             2 * align_up(cap * OD * sizeof(float)) + align_up(2 * cap);
        HIP_TRY(hipMalloc((void**)&p, bytes));
        h->xfer_stage.push_back(p);
        h->xfer_cap = n;
    }
    XferSide st{};
    {
        char* p = h->xfer_stage.back();
        const size_t cap = (size_t)h->xfer_cap;
        const size_t rows_b = align_up((size_t)std::max(SR, std::max(AR, NPHYS + NCOEF)) * cap * sizeof(float));
        st.state = (float*)p; p += rows_b;
        st.aux = (float*)p; p += rows_b;
        st.phys = (float*)p; p += rows_b;
        st.obs = (float*)p; p += align_up(cap * OD * sizeof(float));
        st.final_obs = (float*)p; p += align_up(cap * OD * sizeof(float));
        st.flags = (uint8_t*)p;
        st.stride = h->xfer_cap; st.flag_pitch = h->xfer_cap;
    }
    launch_transfer(XFER_GATHER, st, xfer_side_of(h), D.num_envs, D.num_envs, dst_ids_dev, src_ids_dev, n, err, SR, AR, PR, OD, pot_row,
                    D.hl_goal, D.inv_len_cm, s);
    launch_transfer(XFER_SCATTER, xfer_side_of(h), st, D.num_envs, D.num_envs, dst_ids_dev, src_ids_dev, n, err, SR, AR, PR, OD, -1,
                    D.hl_goal, D.inv_len_cm, s);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_task_transfer_errors(rsx_sim* dst, int64_t* out, void* stream) {
    RSX_ENTER(dst);
    if (dst->P.task == RSX_TASK_NONE) return fail(RSX_ERR_STATE, "no task attached (rsx_task_attach)");
    if (!out) return fail(RSX_ERR_ARG, "out is null");
    hipStream_t s = (hipStream_t)stream;
    uint32_t v = 0;
    HIP_TRY(hipMemcpyAsync(&v, tick_words(dst) + XFER_ERR_WORD, sizeof(v), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(tick_words(dst) + XFER_ERR_WORD, 0, sizeof(uint32_t), s));
    HIP_TRY(hipStreamSynchronize(s));
    *out = (int64_t)v;
    return RSX_OK;
}

}  // extern "C"
