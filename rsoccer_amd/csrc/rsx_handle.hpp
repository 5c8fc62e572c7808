// rsx_handle.hpp — the handle behind the C-ABI (struct rsx_sim) and what the host units (rsx_api*.hip) do with it: error reporting, the entry
// macros, the device guard and a few named helpers.  Private to them: the kernel units never see a handle (rsx_units.hpp: Params, Buffers, scalars).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "rsx.h"
#include "rsx_launch.hpp"
#include "rsx_layout.hpp"
#include "rsx_phys.hpp"
#include "rsx_units.hpp"

struct rsx_sim {
    rsx::Params P;
    rsx::HostModel M;
    int device = 0;
    int field_type = 0, time_step_ms = 0;   // as given to rsx_create (checkpoint header)
    int L = 8;   // lanes per env
    int NR = 0;  // compile-time robot count of the selected kernel variant (0 = generic)
    rsx::StepPlan plan;   // which layout steps the envs (rsx_layout.hpp: plan_layout; set by plan_stepping)
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
    float* d_pcache = nullptr;                // placement cache of the latency-bound batches (rsx_placement.hpp: placement_helper), or null
    unsigned long long* d_pcstats = nullptr;  // [2] cache hits / inline placements (RSX_PCACHE_STATS=1)
    unsigned long long* d_check = nullptr;   // rsx_check_finite counter
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
    // rsx_hot_args.hpp: step_tick) so that captured stepping launches advance it when a graph replays them
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
        rsx::RenderGeom geom;
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

namespace rsx {

inline thread_local std::string g_err;   // rsx_last_error
inline int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            return fail(RSX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)

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

inline size_t align_up(size_t n) { return (n + 255) & ~(size_t)255; }
inline int state_rows(const rsx_sim* h) { return h->P.state_dim + X_ROWS; }
inline size_t state_bytes(const rsx_sim* h) { return (size_t)state_rows(h) * h->P.row_stride * sizeof(float); }   // (with the pad columns)
inline uint32_t* tick_words(const rsx_sim* h) { return reinterpret_cast<uint32_t*>(h->d_metrics); }   // the metrics block as 32-bit words
inline uint32_t* tick_slot0(const rsx_sim* h) { return tick_words(h) + TICK_SLOT_WORD0; }             // ... its per-workgroup step counters

inline Buffers buffers_of(const rsx_sim* h, const float* actions) {
    Buffers b;
    b.state = h->d_state; b.aux = h->d_aux; b.obs = h->d_obs; b.final_obs = h->d_final_obs;
    b.flags = h->d_flags; b.cmds = h->d_cmds; b.actions = actions; b.metrics = h->d_metrics; b.mslots = h->d_mslots;
    b.pcache = h->d_pcache; b.pcstats = h->d_pcstats;
#ifdef RSX_TIMING
    b.dbg = g_dbg;
#endif
    return b;
}

// true while `s` is being captured into a graph (a failed query, e.g. the legacy stream while another one captures, counts as no: the
// launch that follows reports it)
inline bool stream_is_capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
    return cs != hipStreamCaptureStatusNone;
}

// the *_errors calls: the device's count since the last call, cleared as it is read
inline int read_and_clear_word(uint32_t* dev, int64_t* out, hipStream_t s) {
    uint32_t v = 0;
    HIP_TRY(hipMemcpyAsync(&v, dev, sizeof(v), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(dev, 0, sizeof(uint32_t), s));
    HIP_TRY(hipStreamSynchronize(s));
    *out = (int64_t)v;
    return RSX_OK;
}

// a staging allocation of `cap` transfer records at `p` as an XferSide (st null: only the size is wanted); returns its bytes
inline size_t carve_xfer_stage(char* p, size_t cap, int SR, int AR, int OD, XferSide* st = nullptr) {
    const size_t rows_b = align_up((size_t)std::max(SR, std::max(AR, NPHYS + NCOEF)) * cap * sizeof(float));
    const size_t obs_b = align_up(cap * OD * sizeof(float));
    const uintptr_t b = (uintptr_t)p;
    if (st) *st = XferSide{(float*)b, (float*)(b + rows_b), (float*)(b + 2 * rows_b), (float*)(b + 3 * rows_b), (float*)(b + 3 * rows_b + obs_b),
                           (uint8_t*)(b + 3 * rows_b + 2 * obs_b), (int)cap, (int)cap};
    return 3 * rows_b + 2 * obs_b + align_up(2 * cap);
}

// rsx_api.hip: the scan behind every stepping call under RSX_DEBUG_FINITE=1; rsx_api_task.hip: the handle's StepPlan and tick-slot count
int debug_finite(rsx_sim* h, hipStream_t s, const char* where);
void plan_stepping(rsx_sim* h);

}  // namespace rsx
