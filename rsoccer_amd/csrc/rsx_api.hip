// rsx_api.hip — host side of librsx_hip.so: the C-ABI declared in include/rsx.h.  Here: the handle's lifetime, the field, the host-format
// calls and the raw device step; rsx_api_task.hip: the fused tasks; rsx_api_ext.hip: physics, traces, rendering.  No kernel lives in these.
// Stands where the pybind11 module `robosim` stands in the reference (constructed at
// rsoccer_gym/Simulators/rsim.py:116-124,169-177; stepped at :102,:155; read at :105,:158;
// reset at :38; field at :50; destroyed at :41).  HIP only: there is no CPU path in this library.
#include <cstring>

#include "rsx_handle.hpp"

using namespace rsx;

// largest batch whose host-format step (rsx_step / rsx_step_state) lets the kernel read the commands from, and mirror the
// state into, pinned host memory (one launch + one synchronisation; PCIe latency instead of two copy engines' worth of it)
#ifndef RSX_ZERO_COPY_MAX_ENVS
#define RSX_ZERO_COPY_MAX_ENVS 64
#endif

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

// state_out: where the new state is written (nullptr = in place)
// rand_tick >= 0: commands drawn in the kernel with Philox key `seed` (rsx_step_dev_random)
void launch_sim_of(const rsx_sim* h, hipStream_t s, float* state_out = nullptr, int rand_tick = -1, uint64_t seed = 0,
                   const float* cmds_src = nullptr, float* mirror = nullptr) {
    Params P = h->P;
    if (rand_tick >= 0) { P.key0 = (uint32_t)seed; P.key1 = (uint32_t)(seed >> 32); P.env_id_base = 0; }
    Buffers b = buffers_of(h, nullptr);
    if (cmds_src) b.cmds = cmds_src;                      // commands straight from pinned host memory (small batches)
    b.flags = reinterpret_cast<uint8_t*>(mirror);         // the raw step's fourth pointer slot: second copy of the new state, or null
    if (!state_out) state_out = h->d_state;
    if (h->d_phys) launch_sim_phys(P, b, h->L, h->NR, h->d_phys, state_out, rand_tick, s);
    else launch_sim(P, b, h->L, h->NR, state_out, rand_tick, s);
}

// host f64 AoS [B][S'] <-> device f32 SoA [S'][B]
int upload_state(rsx_sim* h, const std::vector<float>& soa, hipStream_t s) {
    h->host_state_valid = false;
    HIP_TRY(hipMemcpyAsync(h->d_state, soa.data(), soa.size() * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    return RSX_OK;
}
int download_state(rsx_sim* h, std::vector<float>& soa, hipStream_t s) {
    soa.resize(state_bytes(h) / sizeof(float));
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
        for (int f = 0; f < state_rows(h); ++f) soa[(size_t)f * S + e] = 0.0f;
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
    const auto dev = [](auto*& p) { if (p) (void)hipFree(p); p = nullptr; };
    const auto pinned = [](auto*& p) { if (p) (void)hipHostFree(p); p = nullptr; };
    pinned(h->pin_cmds); pinned(h->pin_state); pinned(h->wire_cmds); pinned(h->wire_state);
    dev(h->alt_alloc); h->d_state_alt = nullptr;   // (not d_state_alt: after an odd number of flips that is a pointer INTO arena_sim)
    dev(h->d_check); dev(h->d_phys); dev(h->d_trace); dev(h->d_render_err);
    for (auto& rv : h->render_views) (void)hipFree(rv.tpl);
    h->render_views.clear(); h->render_cur = -1;
    for (char* p : h->xfer_stage) (void)hipFree(p);
    h->xfer_stage.clear(); h->xfer_cap = 0;
    dev(h->arena_sim); dev(h->arena_task);
}

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
    auto scan = [&](const float* p, size_t n) { launch_count_nonfinite(p, n, h->d_check, s); };
    scan(h->d_state, (size_t)state_rows(h) * S);
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
int rsx::debug_finite(rsx_sim* h, hipStream_t s, const char* where) {
    static const bool on = std::getenv("RSX_DEBUG_FINITE") != nullptr && std::getenv("RSX_DEBUG_FINITE")[0] == '1';
    if (!on) return RSX_OK;
    if (stream_is_capturing(s)) return fail(RSX_ERR_STATE, "RSX_DEBUG_FINITE=1 scans synchronously and cannot run inside a stream capture");
    int64_t bad = 0;
    if (int rc = check_finite_impl(h, &bad, s)) return rc;
    if (bad) return fail(RSX_ERR_STATE, std::string("RSX_DEBUG_FINITE: ") + std::to_string(bad) + " non-finite value(s) after " + where);
    return RSX_OK;
}

extern "C" {

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
    const size_t sbytes = state_bytes(h);
    const size_t cbytes = (size_t)h->P.n_robots * h->M.cmd_dim * S * sizeof(float);
    if (sbytes >= ((size_t)1 << 32)) {   // the kernels address a row of the state with a 32-bit byte offset (rsx_lane_map.hpp: at_byte)
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
        const size_t wc = B * (size_t)h->P.n_robots * h->M.cmd_dim * sizeof(double), ws = B * (size_t)state_rows(h) * sizeof(double);
        void *dc = nullptr, *ds = nullptr;
        if (B * (size_t)state_rows(h) < ((size_t)1 << 32) &&
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
    std::vector<float> soa(sbytes / sizeof(float), 0.0f);
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
    else soa.assign(state_bytes(h) / sizeof(float), 0.0f);
    apply_reset(h, soa, ball, blue, yellow, env_mask);
    return upload_state(h, soa, s);
}

// the wire-format step of a large batch: commands from h->wire_cmds, new state into h->wire_state (when the host copy is trusted)
static int step_wire_impl(rsx_sim* h, hipStream_t s) {
    const Params& P = h->P;
    const unsigned B = (unsigned)P.num_envs, S = (unsigned)P.row_stride, NC = (unsigned)(P.n_robots * h->M.cmd_dim), rows = (unsigned)state_rows(h);
    h->host_state_valid = false;
    launch_wire_cmds_in(h->wire_cmds_dev, h->d_cmds, B, NC, S, s);
    launch_sim_of(h, s);
    if (h->host_state_cache) launch_wire_state_out(h->d_state, h->wire_state_dev, B, rows, S, s);
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
        launch_sim_of(h, s, nullptr, -1, 0, h->pin_cmds_dev, h->host_state_cache ? h->pin_state_dev : nullptr);
        HIP_TRY(launch_status());
    } else {
        HIP_TRY(hipMemcpyAsync(h->d_cmds, h->pin_cmds, NC * S * sizeof(float), hipMemcpyHostToDevice, s));
        launch_sim_of(h, s);
        HIP_TRY(launch_status());
        if (h->host_state_cache) HIP_TRY(hipMemcpyAsync(h->pin_state, h->d_state, state_bytes(h), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    h->host_state_valid = h->host_state_cache;
    return RSX_OK;
}

static int get_state_impl(rsx_sim* h, double* out, int rows, hipStream_t s) {
    const size_t B = (size_t)h->P.num_envs, S = (size_t)h->P.row_stride;
    if (h->wire_state) {   // large batch: the wire-format copy is made on the device; what is left is a copy out of pinned memory
        const int all = state_rows(h);
        if (!h->host_state_valid) {
            launch_wire_state_out(h->d_state, h->wire_state_dev, (unsigned)B, (unsigned)all, (unsigned)S, s);
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
        HIP_TRY(hipMemcpyAsync(h->pin_state, h->d_state, state_bytes(h), hipMemcpyDeviceToHost, s));
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
    return get_state_impl(h, out, state_rows(h), (hipStream_t)stream);
}

int rsx_set_state(rsx_sim* h, const double* state, void* stream) {
    RSX_ENTER(h);
    if (!state) return fail(RSX_ERR_ARG, "state is null");
    const size_t B = (size_t)h->P.num_envs, S = (size_t)h->P.row_stride;
    const int rows = state_rows(h);
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
    launch_sim_of(h, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return debug_finite(h, (hipStream_t)stream, "rsx_step_dev");
}

static int ensure_alt(rsx_sim* h) {
    if (h->d_state_alt) return RSX_OK;
    const size_t sbytes = state_bytes(h);
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
    for (int i = 0; i < n; ++i) launch_sim_of(h, (hipStream_t)stream, nullptr, (int)(first_tick + (uint32_t)i), seed);
    HIP_TRY(launch_status());
    return debug_finite(h, (hipStream_t)stream, "rsx_step_dev_random");
}

int rsx_step_dev_flip(rsx_sim* h, void* stream) {
    RSX_ENTER(h);
    if (stream_is_capturing((hipStream_t)stream))   // which buffer is current is host state: a replayed graph would keep writing the same one
        return fail(RSX_ERR_STATE, "rsx_step_dev_flip cannot be captured (the buffer roles are host state); capture rsx_step_dev instead");
    if (int rc = ensure_alt(h)) return rc;
    h->host_state_valid = false;
    launch_sim_of(h, (hipStream_t)stream, h->d_state_alt);
    HIP_TRY(launch_status());
    std::swap(h->d_state, h->d_state_alt);
    return debug_finite(h, (hipStream_t)stream, "rsx_step_dev_flip");
}

int rsx_reset_dev(rsx_sim* h, const float* ball_dev, const float* blue_dev, const float* yellow_dev,
                  const uint8_t* env_mask_dev, void* stream) {
    RSX_ENTER(h);
    if (!ball_dev || (h->P.n_blue && !blue_dev) || (h->P.n_yellow && !yellow_dev)) return fail(RSX_ERR_ARG, "null placement array");
    h->host_state_valid = false;
    launch_reset_dev(h->d_state, ball_dev, blue_dev, yellow_dev, env_mask_dev, h->P.num_envs, h->P.row_stride, state_rows(h), h->M.rs,
                     h->P.n_blue, h->P.n_yellow, (float)h->M.field[6], (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_drop_pending_hip_error(void) { return (int)hipGetLastError(); }

int rsx_check_finite(rsx_sim* h, int64_t* n_bad, void* stream) {
    RSX_ENTER(h);
    if (!n_bad) return fail(RSX_ERR_ARG, "n_bad is null");
    return check_finite_impl(h, n_bad, (hipStream_t)stream);
}

}  // extern "C"
